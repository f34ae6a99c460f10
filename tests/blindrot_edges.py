"""The shapes, keys and rows of tests/test_gpu_blindrot_edges.py (host side: no device is needed to build them, and
tests/test_blindrot_host.py checks without one that each has the property it is built for).  The shapes are those of
tests/rgsw_edges.py -- both are instantiations of gadget_fused_kernel and share its domain -- narrowed to what
include/hering_blindrot.h lets he_automorphism_ct_select take; the rows are the schedule edges of he_blind_rotate_core's
batched route.

The project's constants this file leans on, and nothing measured:
  LDS_BYTES   64 KiB of LDS per workgroup: (2 (levelQ + 1) N + N + N / 16) * 8 <= 65536 (hering_rgsw.h, "Routes", which
              hering_blindrot.h refers to for (logN, levelQ + 1)): logN 9 up to 7 Q limbs, logN 10 up to 3, logN 11 one;
  LAST_SHIFT  (nj - 1) pw2 < 64: the last window's shift fits a 64-bit word;
  FILL_WORDS  448 words of two int32 per launch of the selection's fill (launch_tab_fill);
  255 windows at most in a key (he_evk_create_base2)."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from tests import blindrot_ref as BR
from tests import rgsw_edges as E
from tests import rgsw_ref as R

LDS_BYTES, LAST_SHIFT, FILL_WORDS = 65536, 63, 448
Q27 = 0x7FFF801  # the reference's blind rotation modulus (blindrot_test.go:55)


def select_by_header(s, ci=False):
    """whether include/hering_blindrot.h gives he_automorphism_ct_select the shape s (a dict of tests/rgsw_edges.shape): standard
    rings, BaseTwoDecomposition != 0, at most one special prime, the one-launch domain of hering_rgsw.h and every shift below 64"""
    N, nQ = 1 << s["logN"], len(s["q"])
    nj = s["nj"] or R.window_counts(s["q"], s["pw2"]) if s["pw2"] else []
    return (not ci and s["pw2"] != 0 and len(s["p"]) <= 1 and 9 <= s["logN"] <= 11 and nQ <= 8
            and (2 * nQ * N + N + N // 16) * 8 <= LDS_BYTES and all((n - 1) * s["pw2"] <= LAST_SHIFT for n in nj))


def galois_pair(N):
    """two Galois elements of BlindRotateCore's set: g and 2N - g"""
    g = BR.galois_elements(N)
    return [g[0], g[10]]


# ---- A: the lift boundary ---------------------------------------------------------------------------------------------------
def lift_shapes():
    """tests/rgsw_edges.lift_shapes() inside this kernel's domain (pw2 != 0), and the two logN 10 shapes again with pw2 = 7"""
    src = E.lift_shapes()
    out = {k: v for k, v in src.items() if v["pw2"] != 0}
    out["10-p61-pw2-7"] = dict(src["10-p61"], pw2=7)
    out["10-p27-between-pw2-7"] = dict(src["10-p27-between"], pw2=7)
    return out


def planted_key(rng, ringQ, ringP, pw2, component):
    """a Galois key whose gadget product with NTT(1) has tests/rgsw_ref.lift_targets in component `component`'s P accumulator"""
    return R.planted_rgsw(rng, ringQ, ringP, pw2, component)[0]


# ---- B: the edges of the domain ---------------------------------------------------------------------------------------------
def inside_shapes():
    """the largest LDS footprint of each ring degree, the last legal shift and 255 windows"""
    d, s = E.domain_shapes(), E.shift_shapes()
    out = {k: d[k] for k in ("9x7+P", "10x3+P", "10x3", "11x1+P")}
    out.update({k: s[k] for k in ("pw2-7-nj-10", "pw2-9-nj-8")})
    out["beta255"] = E.digit_index_shapes()["beta255"]
    return out


def outside_shapes():
    """{name: (shape, conjugate-invariant)}: the first shape past each LDS bound, shift 64, two special primes (their keys are RNS
    gadgets: BaseTwoDecomposition == 0) and a conjugate-invariant ring"""
    d, s = E.domain_shapes(), E.shift_shapes()
    out = {k: (d[k], False) for k in ("9x8+P", "10x4+P", "11x2+P")}
    out["pw2-8-nj-9"] = (s["pw2-8-nj-9"], False)
    q, p = E.moduli(10, (35, 20), (61, 61))
    out["two-P"] = (E.shape(10, q, p, 0, E.GEN), False)
    q, p = O.GenModuli(12, [35, 20], [61])
    out["conjugate-invariant"] = (E.shape(10, q, p, 7, E.GEN), True)
    return out


# ---- D: moduli --------------------------------------------------------------------------------------------------------------
def moduli_shapes():
    """the one-launch entries of tests/rgsw_edges.moduli_shapes() with bit windows, and (ours) the 9-hiIdD+14|h chain again with
    one window of 61 bits per limb: the mask reaches every modulus, and whole coefficients of the 61-bit limbs -- far beyond four
    times the 14-bit prime, the forward transform's stated input bound -- go into every smaller destination"""
    out = {k: v for k, v in E.moduli_shapes().items() if v["route"] == E.ONE and v["pw2"] != 0}
    out["9-hiIdD+14|h-pw2-61"] = dict(out["9-hiIdD+14|h-pw2-16"], pw2=61)
    return out


# ---- H: schedule edges of the batched core ----------------------------------------------------------------------------------
ROW_LOGN, ROW_N_LWE = 9, 16
ROW_NAMES = ("all-0", "all-1", "all-2N-1", "first-step-positive", "first-step-negative", "last-step-positive", "last-step-negative",
             "flush-coincidences", "beside-the-flush", "random", "flush-coincidences-negative")


def rows(logN=ROW_LOGN, n_lwe=ROW_N_LWE, seed=9900):
    """[11][n_lwe] words mod 2N.  Rows 0-2 share set 0 (csrc/blindrot_plan.h: the sign of 1 / 2N - 1 is lost); 3 and 4 have their
    only set on the first step of the positive / negative walk (k = +-(N/2 - 1)), 5 and 6 on the last (k = +-1); 7 holds the
    discrete logs {10, 20, -10, -20}: the sets at +-20 restart the window's count, so those at +-10 are met directly after the flush
    of a full window; 8 holds {11, -11, 9, -9}, one step beside them; 9 is random; 10 (ours, beyond the issue's ten) holds {-246,
    -236, 251, 242} at logN 9: in each walk one set met with nine steps pending and one directly after a full window's flush."""
    N = 1 << logN
    g = lambda k: pow(BR.GaloisGen, k, 2 * N)
    neg = lambda x: 2 * N - x
    cyc = lambda vals: np.array([vals[i % len(vals)] for i in range(n_lwe)], dtype=np.uint64)
    rng = np.random.default_rng(seed)
    h = N // 2
    return np.stack([cyc([0]), cyc([1]), cyc([2 * N - 1]), cyc([g(h - 1)]), cyc([neg(g(h - 1))]), cyc([g(1)]), cyc([neg(g(1))]),
                     cyc([g(10), g(20), neg(g(10)), neg(g(20))]), cyc([g(11), neg(g(11)), g(9), neg(g(9))]),
                     (rng.integers(0, N, size=n_lwe) * 2 + 1).astype(np.uint64),
                     cyc([neg(g(h - 10)), neg(g(h - 20)), g(h - 5), g(h - 14)])])


def pending_steps(N, ops, j):
    """how the restatement's list reaches the product with key j: the Galois element of the automorphism directly before it (0: the
    list starts with the product, or another product precedes it)"""
    i = ops.index((BR.PROD, j))
    return ops[i - 1][1] if i and ops[i - 1][0] == BR.AUTO else 0


def batch_of(B):
    """indices into rows() of a batch of B entries: the first ten rows in order, then repeats from row 0 (B = 14: ten plus four)"""
    return [b % 10 for b in range(B)]
