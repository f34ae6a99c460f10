"""The cases the encryptor tests share: shapes, seeds, keys and the restatement's result for each (tests/encryptor_ref.py), computed
once.  tests/test_encryptor_host.py runs every case three times -- as is, with exp / log moved 4 ulps up and 4 ulps down -- and asks
for identical words and positions, so that no Gaussian draw a GPU test compares depends on the device's exp / log; a case that
fails that check gets another seed, never a looser comparison."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

from oracle import oracle as O
from tests import encryptor_ref as ER
from tests import sampler_ref as R
from tests.conftest import Pi60, Qi60

XS_P, SIGMA, BOUND = 2 / 3, 3.2, 19.2  # the reference's defaults


@dataclass(frozen=True)
class Case:
    key: str      # "sk" | "pk"
    qp: bool      # an Element[ringqp.Poly]
    logN: int
    nq: int       # limbs of Q
    npp: int      # limbs of P (0: no special primes)
    levelQ: int
    levelP: int   # read for qp only
    batch: int
    seed: int

    @property
    def id(self):
        return f"{self.key}-{'qp' if self.qp else 'q'}-logN{self.logN}-{self.nq}+{self.npp}-l{self.levelQ}.{self.levelP}-b{self.batch}"


# sk and pk, each with and without P; Q element and QP element; a level below the top; batch 1 and 3
ZERO_CASES = [
    Case("sk", False, 5, 2, 0, 1, -1, 1, 101), Case("sk", False, 6, 3, 2, 1, -1, 3, 102), Case("sk", False, 8, 4, 2, 3, -1, 1, 103),
    Case("sk", True, 5, 2, 1, 1, 0, 1, 104), Case("sk", True, 6, 3, 2, 1, 1, 3, 105), Case("sk", True, 7, 3, 2, 2, 0, 1, 106),
    Case("pk", False, 5, 2, 0, 1, -1, 1, 107), Case("pk", False, 6, 3, 0, 1, -1, 3, 108),
    Case("pk", False, 5, 2, 1, 1, -1, 1, 109), Case("pk", False, 6, 3, 2, 1, -1, 3, 110), Case("pk", False, 8, 4, 2, 3, -1, 1, 111),
    Case("pk", True, 5, 2, 1, 1, 0, 1, 112), Case("pk", True, 6, 3, 2, 1, 1, 3, 113),
]
FLAGS = [(1, 1), (1, 0), (0, 1), (0, 0)]  # IsNTT x IsMontgomery
ENCRYPT_CASES = [Case("sk", False, 6, 3, 2, 2, -1, 3, 120), Case("pk", False, 6, 3, 2, 1, -1, 1, 121), Case("pk", False, 6, 2, 0, 1, -1, 1, 122)]
GENPK_CASES = [Case("sk", True, 6, 2, 1, 1, 0, 1, 130), Case("sk", True, 7, 3, 2, 2, 1, 3, 131)]

# two calls on one source, the second under another key: EncryptZero under sk (batch 3), then under pk at another level
SEQUENCE_SEED = 77
SEQUENCE = (ZERO_CASES[1], Case("pk", False, 6, 3, 2, 2, -1, 1, 114))


@functools.lru_cache(maxsize=None)
def rings(logN, nq, npp):
    return O.Ring(1 << logN, Qi60[:nq]), (O.Ring(1 << logN, Pi60[:npp]) if npp else None)


def uniform(rng, moduli, N):
    return np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in moduli])


@functools.lru_cache(maxsize=None)
def keys(c: Case):
    """per entry ((skQ, skP)) or ((pk0Q, pk0P), (pk1Q, pk1P)): uniform words -- every step of an encryption is defined on them"""
    rng = np.random.default_rng(c.seed)
    N, mq, mp = 1 << c.logN, Qi60[:c.nq], Pi60[:c.npp]
    pair = lambda: (uniform(rng, mq, N), uniform(rng, mp, N) if c.npp else None)
    return [pair() if c.key == "sk" else (pair(), pair()) for _ in range(c.batch)]


def run_zero(c: Case, is_ntt, is_mont, exp=math.exp, log=R._log):
    """(the ciphertexts of the restatement [entry][component] = (Q, P), the position of the source afterwards)"""
    oQ, oP = rings(c.logN, c.nq, c.npp)
    src = R.seeded_source(c.seed)
    enc = ER.Encryptor(oQ, oP, src, XS_P, SIGMA, BOUND, exp, log)
    if c.key == "sk":
        out = enc.encrypt_zero_sk(keys(c), c.levelQ, c.levelP if c.qp else -1, is_ntt, is_mont, c.batch)
    elif not c.qp and not c.npp:
        out = enc.encrypt_zero_pk_nop(keys(c), c.levelQ, is_ntt, c.batch)
    else:
        out = enc.encrypt_zero_pk(keys(c), c.levelQ, c.levelP, c.qp, is_ntt, is_mont, c.batch)
    return out, src.pos


@functools.lru_cache(maxsize=None)
def want_zero(c: Case, is_ntt, is_mont):
    return run_zero(c, is_ntt, is_mont)


def run_sequence(exp=math.exp, log=R._log):
    """([the ciphertexts of each call of SEQUENCE, IsNTT and not IsMontgomery], the position of the source after both)"""
    c1, c2 = SEQUENCE
    oQ, oP = rings(c1.logN, c1.nq, c1.npp)
    src = R.seeded_source(SEQUENCE_SEED)
    enc = ER.Encryptor(oQ, oP, src, XS_P, SIGMA, BOUND, exp, log)
    w1 = enc.encrypt_zero_sk(keys(c1), c1.levelQ, -1, 1, 0, c1.batch)
    w2 = enc.encrypt_zero_pk(keys(c2), c2.levelQ, -1, False, 1, 0, c2.batch)
    return [w1, w2], src.pos


def same(a, b):
    """two results of run_zero, word for word and position for position"""
    if a[1] != b[1]:
        return False
    for ea, eb in zip(a[0], b[0]):
        for (qa, pa), (qb, pb) in zip(ea, eb):
            if not np.array_equal(qa, qb) or (pa is None) != (pb is None) or (pa is not None and not np.array_equal(pa, pb)):
                return False
    return True


# ---- real keys (the end-to-end and the host properties) ------------------------------------------------------------------------------
def ternary_secret(rng, oQ, oP):
    """(the signed coefficients, sk.Value.Q, sk.Value.P): NTT and Montgomery, as the reference holds a secret key"""
    N = oQ.N
    s = rng.integers(-1, 2, N)
    to = lambda ring: ring.unop("MForm", ring.NTT(np.stack([np.where(s < 0, np.uint64(q - 1), s.astype(np.uint64) & np.uint64(1)) for q in ring.moduli])))
    return s, to(oQ), (to(oP) if oP is not None else None)


def centered(words, q):
    """the signed representatives of one limb"""
    w = [int(x) % q for x in words]
    return [x - q if x > q // 2 else x for x in w]


def negacyclic(a, b):
    """a * b in Z[X]/(X^N + 1) on Python integers"""
    N = len(a)
    out = [0] * N
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                if i + j < N:
                    out[i + j] += x * y
                else:
                    out[i + j - N] -= x * y
    return out
