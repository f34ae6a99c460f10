"""Case tables and input builders of the small-ring transform and rescale edge tests (host side: shared by
tests/test_gpu_ntt_edges.py and checked without a GPU in tests/test_ntt_edges_host.py).

The stand-alone transforms are three kernels chosen per modulus (double precision below 2^47, correction-free integer below 2^58,
forward only, Harvey form up to 2^61), each instantiated for the row sizes 2^4 .. 2^13, with a partial round where the row size
is no multiple of four stages and workgroups of one and two threads at 2^4 and 2^5.  The chains here put the primes nearest to
each class threshold, and the smallest NTT-friendly prime there is, on every one of those row sizes."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from tests.boundary import CANONICAL_KINDS, WORST_CASE_KINDS, WordCycle, class_chain, wild_words, word_row
from tests.helpers import rng_for

ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
SENTINEL = np.uint64(0xA5A5A5A5DEADBEEF)  # what the limbs above a level must keep (no valid word of a chain here: above 2^63)

TRANSFORM_LETTERS = "ddDiiIhh"


def log_root(logN: int, ci: bool) -> int:
    """log2 of the root order: 2N for a standard ring, 4N for a conjugate-invariant one"""
    return logN + (2 if ci else 1)


def floor_prime(lr: int) -> int:
    """the smallest prime = 1 mod 2^lr (97, 257, 7681, 12289, 40961, 65537, ...: the plaintext moduli of the encoder's ringT)"""
    q = (1 << lr) + 1
    while not O.IsPrime(q):
        q += 1 << lr
    return q


def transform_chain(logN: int, ci: bool):
    """nine limbs: two at the double-precision edge, one just above it, two at the correction-free edge, one just above it, two
    at the Harvey edge, and the floor prime.  Every prefix of three or more limbs holds a class change."""
    lr = log_root(logN, ci)
    return class_chain(lr - 1, TRANSFORM_LETTERS) + [floor_prime(lr)]


# (conjugate-invariant, logN): every single-pass row size 2^4 .. 2^12 of both ring types, and the column passes of one and two
# stages over rows of 2^12 (logN 13, 14)
TRANSFORM_CASES = [(False, n) for n in range(4, 15)] + [(True, n) for n in range(4, 14)]
# five column stages in one pass
BIG_LOGN, BIG_LETTERS, BIG_KINDS = 18, "dDiIh", ("max_lazy", "uniform_lazy")


def case_id(case) -> str:
    return f"{'ci' if case[0] else 'std'}-{case[1]}"


def first_batch(rng, mods, N, kinds=WORST_CASE_KINDS) -> np.ndarray:
    """[kinds][limbs][N]: one polynomial per worst-case kind, the entries of ONE batch (words below 2q: the reference's domain)"""
    return np.stack([np.stack([word_row(kind, rng, m, N) for m in mods]) for kind in kinds])


def second_batch(oring, spectra_of, rng, nlimbs, N) -> np.ndarray:
    """[len(spectra_of) + 2][limbs][N]: the oracle's NTT of the given polynomials (dense, full-range spectra for the inverse
    side), arbitrary 64-bit words, and 2^64 - 1 everywhere (outside the reference's domain: the public entries reduce first)"""
    return np.stack([oring.NTT(p) for p in spectra_of] + [wild_words(rng, (nlimbs, N)), np.full((nlimbs, N), ALL_ONES, dtype=np.uint64)])


def transform_inputs(case):
    """(moduli, first batch, second batch, number of spectra leading the second batch) of a case of TRANSFORM_CASES or "big" """
    if case == "big":
        ci, logN, mods, kinds = False, BIG_LOGN, class_chain(BIG_LOGN, BIG_LETTERS), BIG_KINDS
    else:
        ci, logN = case
        mods, kinds = transform_chain(logN, ci), WORST_CASE_KINDS
    N = 1 << logN
    rng = rng_for(7100 + 32 * int(ci) + logN)
    x1 = first_batch(rng, mods, N, kinds)
    oring = O.Ring(N, mods, ci)
    x2 = second_batch(oring, [x1[0], x1[1]], rng, len(mods), N)
    return mods, x1, x2, 2


# which row kernel a limb gets: one- and two-thread workgroups, a partial round, the largest single-pass ring, rows under a
# column pass, and a conjugate-invariant ring
DISPATCH_CASES = [(False, 4), (False, 5), (False, 9), (False, 12), (False, 13), (True, 6)]


def expected_dispatch(mods):
    """(limbs of the double-precision class, the integer classes present) by the thresholds 2^47 / 2^58 restated in
    tests/boundary.py: a forward row launch splits into one launch per class, an inverse one into double precision and Harvey"""
    from tests.boundary import modulus_class

    cls = [modulus_class(m) for m in mods]
    return cls.count(0), sorted({c for c in cls if c > 0})


def reduce_words(x: np.ndarray, mods) -> np.ndarray:
    """x mod q limb by limb ([..., limbs, N]), on the host"""
    q = np.array(mods, dtype=np.uint64).reshape((len(mods), 1))
    return x % q


# ---------------------------------------------------------------------------------------------------------------
# the entry-pairing route of the inverse double-precision kernel
# ---------------------------------------------------------------------------------------------------------------
# (conjugate-invariant, logN, batch): three double-precision limbs.  3 x 2049 = 6147 and, with the two rows per limb of logN 13,
# 3 x 1025 x 2 = 6150 workgroups -- just over the threshold at which a workgroup takes two entries; odd batches, so that the last
# workgroup holds a single entry.  logN 4 with batch 1 and 2: the one-thread workgroup below the threshold, and the batch of one
# that the clamp of the pairing to the batch is there for.
PAIRING_CASES = [(False, 4, 2049), (False, 5, 2049), (False, 8, 2049), (False, 11, 2049), (False, 13, 1025), (True, 8, 2049),
                 (False, 4, 1), (False, 4, 2)]
PAIRING_THRESHOLD = 6144


def pairing_id(case) -> str:
    return f"{'ci' if case[0] else 'std'}-{case[1]}-b{case[2]}"


def pairing_chain(logN: int, ci: bool):
    return class_chain(log_root(logN, ci) - 1, "ddd")


def pairing_workgroups(logN: int, batch: int, nlimbs: int = 3) -> int:
    """workgroups of the inverse row launch before pairing: batch x limbs x rows per limb (one row up to logN 12, rows of 2^12
    up to logN 15, of 2^13 above)"""
    return batch * nlimbs * (1 << (0 if logN <= 12 else logN - 12 if logN <= 15 else logN - 13))


def pairing_inputs(case) -> tuple:
    ci, logN, batch = case
    mods = pairing_chain(logN, ci)
    rng, cyc = rng_for(7300 + 32 * int(ci) + logN + batch), WordCycle(WORST_CASE_KINDS)
    return mods, np.stack([cyc(rng, mods, 1 << logN) for _ in range(batch)])


def pairing_sample(batch: int):
    return sorted({b for b in (0, 1, 2, 3, batch // 2, batch - 2, batch - 1) if 0 <= b < batch})


# ---------------------------------------------------------------------------------------------------------------
# rescale on single-pass rings
# ---------------------------------------------------------------------------------------------------------------
RESCALE_LETTERS = ("didhdId", "hidi")
# (conjugate-invariant, logN, letters)
RESCALE_CASES = [(ci, n, letters) for ci, sizes in ((False, (4, 5, 8, 11, 12)), (True, (4, 10))) for n in sizes for letters in RESCALE_LETTERS]
RESCALE_BATCH = 2
MAX_EXTRA_POLYS = 4096


def rescale_id(case) -> str:
    return f"{'ci' if case[0] else 'std'}-{case[1]}-{case[2]}"


def rescale_chain(case):
    ci, logN, letters = case
    return class_chain(log_root(logN, ci) - 1, letters)


def extreme_polys(oring, rng, mods, N):
    """the polynomials of the descent: the canonical worst-case kinds as NTT-domain words, and the transforms of the
    coefficient-domain all-(q - 1) and alternating polynomials, so that the inverse transform's OUTPUT is extreme too"""
    polys = [np.stack([word_row(kind, rng, m, N) for m in mods]) for kind in CANONICAL_KINDS]
    return polys + [oring.NTT(polys[0]), oring.NTT(polys[1])]


def lazy_top_words(oring, polys) -> int:
    """how many words of the oracle's INTTLazy of the top limb are at or above q_L over these polynomials (on a
    conjugate-invariant ring the NTT-domain rescale hands exactly those words to the other moduli)"""
    top, qL = len(oring.moduli) - 1, np.uint64(oring.moduli[-1])
    return sum(int((oring.INTTLazy(p)[top] >= qL).sum()) for p in polys)


def rescale_inputs(case):
    """(moduli, polynomials) of a case of RESCALE_CASES: an even number of polynomials, run RESCALE_BATCH at a time.  On a
    conjugate-invariant ring, pairs of uniform polynomials are added until the oracle's INTTLazy of the top limb has held a
    word at or above q_L (about one word in a thousand: many polynomials at N = 16)."""
    ci, logN, _ = case
    mods, N = rescale_chain(case), 1 << logN
    rng = rng_for(7500 + 32 * int(ci) + logN + len(mods))
    oring = O.Ring(N, mods, ci)
    polys = extreme_polys(oring, rng, mods, N)
    if ci:
        seen = lazy_top_words(oring, polys)
        while seen == 0 and len(polys) < MAX_EXTRA_POLYS:
            extra = [np.stack([word_row("uniform", rng, m, N) for m in mods]) for _ in range(RESCALE_BATCH)]
            seen += lazy_top_words(oring, extra)
            polys += extra
    return mods, polys


def rescale_descent(pr, polys, B, ci=False, coeff_top=False):
    """DivRound / DivFloorByLastModulusNTT down the whole chain of the Pair `pr`, B polynomials at a time: ...ManyNTT with
    nb = 2 from the top, then level by level out of place and in place (p1 aliasing p0) on the descent's own outputs, and the
    extreme words themselves afresh at every level; every word against the oracle.  coeff_top adds the coefficient-domain
    variants (and their ...Many forms, nb = 2) at the top level."""
    import lattigo_amd as la

    qs, top = pr.q, len(pr.q) - 1
    for c0 in range(0, len(polys), B):
        xs = np.stack(polys[c0 : c0 + B])
        for name in ("DivRoundByLastModulusNTT", "DivFloorByLastModulusNTT"):
            cur = xs.copy()
            pin = pr.up(pr.gQ, cur, batch=B)
            many = name.replace("NTT", "ManyNTT")
            want = np.stack([getattr(pr.oQ, many)(2, cur[b]) for b in range(B)])
            po = la.Poly(pr.gQ, len(qs), B)
            getattr(pr.gQ, many)(2, pin, po)
            assert np.array_equal(po.get()[:, : top - 1], want), (many, c0)
            for level in range(top, 0, -1):
                sub = O.Ring(pr.N, pr.q[: level + 1], ci)
                want = np.stack([getattr(sub, name)(cur[b, : level + 1]) for b in range(B)])
                po = la.Poly(pr.gQ, len(qs), B)
                getattr(pr.gQ.AtLevel(level), name)(pin, po)
                assert np.array_equal(po.get()[:, :level], want), (name, c0, level, "out of place")
                getattr(pr.gQ.AtLevel(level), name)(pin, pin)
                assert np.array_equal(pin.get()[:, :level], want), (name, c0, level, "in place")
                cur = np.concatenate([want, cur[:, level:]], axis=1)
                # and the extreme words themselves at this level (the descent above hands its own outputs down)
                want = np.stack([getattr(sub, name)(xs[b, : level + 1]) for b in range(B)])
                pfresh = pr.up(pr.gQ, xs, batch=B)
                getattr(pr.gQ.AtLevel(level), name)(pfresh, pfresh)
                assert np.array_equal(pfresh.get()[:, :level], want), (name, c0, level, "extreme words, in place")
        if coeff_top:
            for name in ("DivRoundByLastModulus", "DivFloorByLastModulus"):
                for nb in (1, 2):
                    fn = name if nb == 1 else name + "Many"
                    args = () if nb == 1 else (nb,)
                    want = np.stack([getattr(pr.oQ, fn)(*args, xs[b]) for b in range(B)])
                    po = la.Poly(pr.gQ, len(qs), B)
                    getattr(pr.gQ, fn)(*args, pr.up(pr.gQ, xs, batch=B), po)
                    assert np.array_equal(po.get()[:, : top + 1 - nb], want), (fn, c0, "out of place")
                    pin = pr.up(pr.gQ, xs, batch=B)
                    getattr(pr.gQ, fn)(*args, pin, pin)
                    assert np.array_equal(pin.get()[:, : top + 1 - nb], want), (fn, c0, "in place")
