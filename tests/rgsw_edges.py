"""The shapes, primes and words of tests/test_gpu_rgsw_edges.py (host side: no device is needed to build them, and
tests/test_rgsw_host.py checks without one that each has the property it is built for).

A shape is a dict: logN, q, p (moduli), pw2, route ("one-launch" / "generic": what include/hering_rgsw.h says the shape takes)
and optionally nj (window counts other than the reference's)."""
from __future__ import annotations

import math

import numpy as np

from oracle import oracle as O
from tests import boundary as Bd
from tests import rgsw_ref as R

ONE, GEN = "one-launch", "generic"
Q14 = 12289  # 3 * 2^12 + 1: NTT-friendly up to logN 11, smaller than a 14-bit window's mask


def moduli(logN, logq, logp=()):
    q, p = O.GenModuli(logN + 1, list(logq), list(logp))
    return list(q), list(p)


def shape(logN, q, p, pw2, route, nj=None):
    return dict(logN=logN, q=list(q), p=list(p), pw2=pw2, route=route, nj=nj)


def fused_by_header(logN, nQ, nP):
    """the one-launch domain as include/hering_rgsw.h states it (standard rings, levelP < 1)"""
    N = 1 << logN
    return 9 <= logN <= 11 and nQ <= 8 and nP <= 1 and (2 * nQ * N + N + N // 16) * 8 <= 65536


# ---- B: the edges of the one-launch domain --------------------------------------------------------------------------------------
_B_BITS = (35, 20, 45, 27, 50, 30, 40, 25)


def domain_shapes():
    out = {}
    q9, p9 = moduli(9, _B_BITS, (61,))
    out["9x7+P"] = shape(9, q9[:7], p9, 13, ONE)
    out["9x8+P"] = shape(9, q9, p9, 13, GEN)
    q10, p10 = moduli(10, _B_BITS[:4], (61,))
    out["10x3+P"] = shape(10, q10[:3], p10, 13, ONE)
    out["10x3"] = shape(10, q10[:3], [], 13, ONE)
    out["10x4+P"] = shape(10, q10, p10, 13, GEN)
    q11, p11 = moduli(11, _B_BITS[:2], (61,))
    out["11x1+P"] = shape(11, q11[:1], p11, 7, ONE)
    out["11x2+P"] = shape(11, q11, p11, 7, GEN)
    return out


def digit_index_shapes():
    """logN 9, pw2 = 1: one window per bit.  "beta255": 255 windows in all, the most he_evk_create_base2 takes -- the largest digit
    index the kernel's uint8_t prefix[] + j can be asked for is 254.  "prefix255" has prefix[levelQ] == 255 and "prefix256" more:
    both need 256 or more windows."""
    h = Bd.primes_below(61, 10, 4)            # four 61-bit primes
    s60 = Bd.primes_below(60, 10, 3)          # three 60-bit primes
    out = {"beta255": shape(9, [s60[0], s60[1], s60[2], h[0], Q14], [], 1, ONE),        # 60 + 60 + 60 + 61 + 14
           "prefix255": shape(9, [s60[0], s60[1], s60[2], h[0], Q14, h[1]], [], 1, None),
           "prefix256": shape(9, [h[2], s60[1], s60[2], h[0], Q14, h[1]], [], 1, None)}
    return out


def shift_shapes():
    """(nj - 1) pw2 at 63 (one-launch) and at 64, the first value that fails the bound (generic): keys with more windows than the
    limb has bits -- he_evk_create_base2 takes nj pw2 <= 64 + pw2 -- whose upper windows are windows of zero"""
    q, p = moduli(9, (35,), (61,))
    return {"pw2-7-nj-10": shape(9, q, p, 7, ONE, nj=[10]), "pw2-9-nj-8": shape(9, q, p, 9, ONE, nj=[8]),
            "pw2-8-nj-9": shape(9, q, p, 8, GEN, nj=[9]), "pw2-16-nj-5": shape(9, q, p, 16, GEN, nj=[5])}


# ---- D: moduli --------------------------------------------------------------------------------------------------------------
def moduli_shapes():
    out = {}
    # one-launch: every class letter, the 14-bit prime as a source and as a destination below / above the mask
    q9 = Bd.class_chain(9, "hiIdD") + [Q14]
    p9 = Bd.class_chain(9, "h", skip={"h": 1})
    out["9-hiIdD+14|h-pw2-13"] = shape(9, q9, p9, 13, ONE)   # mask 8191 < 12289: no destination is reduced
    out["9-hiIdD+14|h-pw2-14"] = shape(9, q9, p9, 14, ONE)   # mask 16383 >= 12289 for that one destination only
    out["9-hiIdD+14|h-pw2-16"] = shape(9, q9, p9, 16, ONE)   # mask 65535 >= 4 * 12289: windows above the transform's input bound
    out["9-hiIdD+14|h-all-ones"] = shape(9, q9, p9, 0, ONE)  # whole coefficients of 61-bit limbs into the 14-bit destination
    out["10-hd+14|i"] = shape(10, Bd.class_chain(10, "hd") + [Q14], Bd.class_chain(10, "i"), 14, ONE)
    out["10-IDi"] = shape(10, Bd.class_chain(10, "IDi"), [], 13, ONE)
    out["11-I|h"] = shape(11, Bd.class_chain(11, "I"), Bd.class_chain(11, "h"), 0, ONE)
    out["11-14|D"] = shape(11, [Q14], Bd.class_chain(11, "D"), 13, ONE)
    # generic, logN 12: all three classes in Q
    q12 = Bd.class_chain(12, "dihDI")
    out["12-dihDI|i"] = shape(12, q12, Bd.class_chain(12, "i", skip={"i": 1}), 13, GEN)
    out["12-dihDI|h"] = shape(12, q12, Bd.class_chain(12, "h", skip={"h": 1}), 0, GEN)
    out["12-dihd|ih"] = shape(12, Bd.class_chain(12, "dihd"), Bd.class_chain(12, "ih", skip={"i": 1, "h": 1}), 0, GEN)  # branch M
    return out


# ---- A: the lift boundary ----------------------------------------------------------------------------------------------------
def lift_shapes():
    out = {}
    for logN in (9, 10, 11):
        nq = 1 if logN == 11 else 2
        q, _ = moduli(logN, (35, 36)[:nq])
        out[f"{logN}-p61"] = shape(logN, q, Bd.primes_below(61, logN + 1, 1), 7 if logN != 10 else 0, ONE)
        _, p20 = moduli(logN, (), (20,))
        out[f"{logN}-p20-below-q"] = shape(logN, q, p20, 7, ONE)
    for logN in (9, 10):
        q, p = moduli(logN, (35, 20), (27,))
        out[f"{logN}-p27-between"] = shape(logN, q, p, 7 if logN == 9 else 0, ONE)
    return out


# ---- I: the 32-bit branch's wrap bound ---------------------------------------------------------------------------------------
def wrap_primes(logN=10):
    """Two NTT-friendly primes on either side of 2^32 / sqrt(120) ~ 2^28.55: with pw2 = 3 both have D = 10 windows and
    2 D (6q - 2)(q - 1) < 2^64 holds for the smaller one only; pw2 = 1, 2 fail and pw2 = 4..8 hold for both"""
    edge, step = math.isqrt((1 << 64) // 120), 2 << logN
    lo = edge - edge % step + 1
    while lo > edge or not O.IsPrime(lo):
        lo -= step
    hi = lo + step
    while not O.IsPrime(hi):
        hi += step
    return lo, hi


# ---- E: words ------------------------------------------------------------------------------------------------------------
COEFF_KINDS = ("coeff_max", "coeff_mask", "coeff_zero")
CT_KINDS = ("max", "alt", "alt_lazy", "half", "max_lazy", "uniform_lazy") + COEFF_KINDS


def coeffs(kind, mods, N, pw2):
    """[limbs, N] coefficient-domain worst cases: all q - 1; every window equal to the mask with the top one partial; zero"""
    if kind == "coeff_max":
        return np.stack([np.full(N, int(m) - 1, dtype=np.uint64) for m in mods])
    if kind == "coeff_mask":
        return np.stack([R.all_mask_coeffs(m, pw2, N) if pw2 else np.full(N, int(m) - 1, dtype=np.uint64) for m in mods])
    if kind == "coeff_zero":
        return np.zeros((len(mods), N), dtype=np.uint64)
    raise ValueError(kind)


class CtCycle:
    """Polynomials of a ciphertext, one kind of CT_KINDS per call in turn (tests/boundary.py's WordCycle with the
    coefficient-domain kinds, uploaded as NTT(c), added)"""

    def __init__(self, ring: O.Ring, pw2: int, start: int = 0):
        self.ring, self.pw2, self.k = ring, pw2, start

    def __call__(self, rng, mods, N):
        kind = CT_KINDS[self.k % len(CT_KINDS)]
        self.k += 1
        if kind in COEFF_KINDS:
            return R._at(self.ring, 0, len(mods)).NTT(coeffs(kind, mods, N, self.pw2))
        return np.stack([Bd.word_row(kind, rng, m, N) for m in mods])
