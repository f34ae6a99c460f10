"""The cases the key-generator tests share: shapes, seeds, secret keys and the restatement's result for each (tests/keygen_ref.py),
computed once.  tests/test_keygen_host.py runs every case three times -- as is, with exp / log moved 4 ulps up and 4 ulps down --
and asks for identical words and positions, so that no Gaussian draw a GPU test compares depends on the device's exp / log; a case
that fails that check gets another seed, never a looser comparison."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

from oracle import oracle as O
from tests import boundary
from tests import keygen_ref as KR
from tests import sampler_ref as R
from tests.conftest import Pi60, Qi60

XS_P, SIGMA, BOUND = 2 / 3, 3.2, 19.2  # the reference's defaults


@dataclass(frozen=True)
class Case:
    name: str
    logN: int
    Q: tuple      # the evaluator's Q chain
    P: tuple      # its special primes (empty: none)
    levelQ: int   # the key's levels
    levelP: int
    pw2: int
    seed: int
    ci: bool = False

    @property
    def id(self):
        return self.name

    @property
    def N(self):
        return 1 << self.logN

    @property
    def rows(self):
        return len(KR.gadget_rows(self.Q, self.levelQ, self.levelP, self.pw2))


def _case(name, logN, Q, P, seed, levelQ=None, levelP=None, pw2=0, ci=False):
    return Case(name, logN, tuple(Q), tuple(P), len(Q) - 1 if levelQ is None else levelQ, len(P) - 1 if levelP is None else levelP, pw2, seed, ci)


C_3P2 = _case("3+2-partial-digit", 5, Qi60[:3], Pi60[:2], 201)            # beta = 2, the last digit partial: the break of :218
C_4P2 = _case("4+2-divides", 6, Qi60[:4], Pi60[:2], 202)
C_3P1 = _case("3+1-beta3", 5, Qi60[:3], Pi60[:1], 203)
C_LOW = _case("4+2-key-at-2.0", 6, Qi60[:4], Pi60[:2], 204, levelQ=2, levelP=0)  # a key below the evaluator's top levels
C_B16 = _case("2+1-pw2-16", 5, Qi60[:2], Pi60[:1], 205, pw2=16)
C_B7 = _case("2+1-pw2-7", 5, Qi60[:2], Pi60[:1], 206, pw2=7)
C_B16_NOP = _case("2+0-pw2-16", 5, Qi60[:2], (), 207, pw2=16)
C_CLASS = _case("classes-dih+h", 6, boundary.class_chain(6, "dih"), boundary.class_chain(6, "h", skip={"h": 1}), 208)
# a modulus just above 2^47: its mask is 2^48 - 1 and about half of the uniform words of that limb are rejected
C_REJECT = _case("rejecting-modulus", 6, [boundary.primes_above(47, 7, 1)[0], Qi60[0]], Pi60[:1], 209)
C_BIG = _case("logN13-2+1", 13, Qi60[:2], Pi60[:1], 210)                    # the two-launch transform
C_CI = _case("conjugate-invariant-2+1", 6, Qi60[:2], Pi60[:1], 211, ci=True)
C_SWITCH = _case("ring-switch-5-7", 7, Qi60[:3], Pi60[:1], 212)            # GenEvaluationKey between a logN 5 key and a logN 7 key
SMALL_LOGN = 5

RLK_CASES = [C_3P2, C_4P2, C_3P1, C_LOW, C_B16, C_B7, C_B16_NOP, C_CLASS, C_REJECT, C_BIG]
GALOIS_CASES = [C_3P2, C_CI]
GALOIS_SET_CASE = C_3P1
SK_CASES = [C_3P2, C_B16_NOP]  # with and without P
GADGET_CASES = [c for c in RLK_CASES if c is not C_BIG]


def galois_elements(c: Case):
    """5, its inverse, and NthRoot - 1.  A conjugate-invariant ring has the automorphisms 5^k alone: for NthRoot - 1 the reference's
    AutomorphismNTTIndex(N, 4N, .) holds positions in [N, 2N) and its AutomorphismNTTWithIndex panics; the device refuses it"""
    nth = (4 if c.ci else 2) * c.N
    return [5, pow(5, -1, nth)] + ([] if c.ci else [nth - 1])


def sk_hw(c: Case):
    return c.N // 4 + 1


@functools.lru_cache(maxsize=None)
def rings(c: Case):
    return O.Ring(c.N, c.Q, c.ci), (O.Ring(c.N, c.P, c.ci) if c.P else None)


def generator(c: Case, seed, exp=math.exp, log=R._log):
    oQ, oP = rings(c)
    src = R.seeded_source(seed)
    return KR.KeyGenerator(oQ, oP, src, XS_P, SIGMA, BOUND, exp, log), src


@functools.lru_cache(maxsize=None)
def secret(c: Case):
    """the secret key the evaluation keys of a case are generated for: the restatement's own, at the evaluator's top levels, from a
    source of its own (the density sampler walks bits: no exp / log)"""
    kg, _ = generator(c, c.seed + 5000)
    return kg.gen_secret_key(len(c.Q) - 1, len(c.P) - 1)


def run_rlk(c: Case, exp=math.exp, log=R._log):
    """(key, the Gaussians of its rows, the position of the source afterwards, (skIn, skOut))"""
    kg, src = generator(c, c.seed, exp, log)
    key = kg.gen_relinearization_key(secret(c), c.levelQ, c.levelP, c.pw2)
    return key, kg.gaussians[0], src.pos, kg.operands[0]


def run_galois(c: Case, galEl, exp=math.exp, log=R._log):
    kg, src = generator(c, c.seed + 100 + galEl % 89, exp, log)
    key = kg.gen_galois_key(galEl, secret(c), c.levelQ, c.levelP, c.pw2)
    return key, kg.gaussians[0], src.pos, kg.operands[0]


def run_galois_set(c: Case, exp=math.exp, log=R._log):
    """three keys on one source: (keys, Gaussians per key, position, (skIn, skOut) per key)"""
    kg, src = generator(c, c.seed + 300, exp, log)
    keys = kg.gen_galois_keys(galois_elements(c), secret(c), c.levelQ, c.levelP, c.pw2)
    return keys, kg.gaussians, src.pos, kg.operands


@functools.lru_cache(maxsize=None)
def small_secret(c: Case):
    """sk.Value.Q of a secret key of the ring of degree 2^SMALL_LOGN over the same Q chain"""
    oq = O.Ring(1 << SMALL_LOGN, c.Q)
    return KR.KeyGenerator(oq, None, R.seeded_source(c.seed + 6000), XS_P, SIGMA, BOUND).gen_secret_key(len(c.Q) - 1, -1)[0]


def run_switch(c: Case, up: bool, exp=math.exp, log=R._log):
    """GenEvaluationKey in the large ring, up: from the small key to the large one; else the other way"""
    kg, src = generator(c, c.seed + 500 + int(up), exp, log)
    a, b = (small_secret(c), secret(c)[0]) if up else (secret(c)[0], small_secret(c))
    key = kg.gen_evaluation_key_sk(a, b, c.levelQ, c.levelP, c.pw2)
    return key, kg.gaussians[0], src.pos, kg.operands[0]


def run_sk(c: Case, hw):
    """hw None: the density sampler.  (sk, position)"""
    kg, src = generator(c, c.seed + 400 + (hw or 0))
    sk = kg.gen_secret_key(len(c.Q) - 1, len(c.P) - 1) if hw is None else kg.gen_secret_key_hw(hw, len(c.Q) - 1, len(c.P) - 1)
    return sk, src.pos


want_rlk = functools.lru_cache(maxsize=None)(lambda c: run_rlk(c))
want_galois = functools.lru_cache(maxsize=None)(lambda c, galEl: run_galois(c, galEl))
want_galois_set = functools.lru_cache(maxsize=None)(lambda c: run_galois_set(c))
want_switch = functools.lru_cache(maxsize=None)(lambda c, up: run_switch(c, up))
want_sk = functools.lru_cache(maxsize=None)(lambda c, hw: run_sk(c, hw))


def uniform_poly(c: Case, salt: int):
    """[limbs of Q][N] canonical uniform words"""
    rng = np.random.default_rng([c.seed, salt])
    return np.stack([rng.integers(0, q, c.N, dtype=np.uint64) for q in c.Q])


def same_key(a, b):
    return np.array_equal(a["q"], b["q"]) and np.array_equal(a["p"], b["p"])
