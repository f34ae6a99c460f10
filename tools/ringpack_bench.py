#!/usr/bin/env python3
"""Times the ring-packing entries (include/hering_ringpack.h, lattigo_amd.rlwe.RingPackingEvaluator) against the reference's own
sequence of calls (core/rlwe/ring_packing.go) composed from the entry points the library had before them: ApplyEvaluationKey,
SwitchCiphertextRingDegreeNTT, MulCoeffsMontgomery[ThenAdd] by a monomial table held as a polynomial, Add, Sub, CopyLvl and one
Automorphism per ciphertext.  The composed legs use none of the new symbols (the monomial tables are built on the host from
Ring.roots), so `--composed-only` runs them on a build that does not have the feature.

    python tools/ringpack_bench.py [--case split16 split13 expand repack] [--reps 10]

  split16 / split13   Split and Merge at logN 16 -> 15 with the c5 shape's 25 + 5 moduli, and at 13 -> 12 (6 + 2), batch 1 and 32
  expand              one Expand at logN 11, logGap 0, 2 + 1 limbs (2048 outputs)
  repack              one Repack (Pack) of 2^11 ciphertexts at logN 11

Every fused result is compared word for word with the composed one outside the timed region; the exit status is non-zero
when one differs or when a fused form is slower than its composed sequence.  Kernel figures come from
he_prof_end_bytes (HIP events around each launch, the bytes each launcher accounts); the fraction of peak HBM is over 8 TB/s.
Prints one JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import lattigo_amd as la  # noqa: E402
from lattigo_amd import rlwe as R  # noqa: E402
from oracle import oracle as O  # noqa: E402

PEAK_HBM = 8.0e12
C5_LOGQ = [60] + [40] * 9 + [39] * 3 + [60] * 8 + [56] * 4
C5_LOGP = [61] * 5
KERNELS = ("ring_split", "ring_merge", "expand_step", "pack_pre", "pack_post", "xpow2_fill")


def rand_polys(rng, q, N, B):
    return np.stack([np.stack([rng.integers(0, qi, size=N, dtype=np.uint64) for qi in q]) for _ in range(B)])


def random_key(rng, gev, q, p, N):
    beta = O.BaseRNSDecompositionVectorSize(len(q) - 1, len(p) - 1)
    kq = np.stack([np.stack([rand_polys(rng, q, N, 1)[0] for _ in range(2)]) for _ in range(beta)])
    kp = np.stack([np.stack([rand_polys(rng, p, N, 1)[0] for _ in range(2)]) for _ in range(beta)])
    return gev.NewEvaluationKey(kq, kp)


def xpow2_host(ring, i, div):
    """XPow2NTT[i] / XInvPow2NTT[i] from the ring's twiddles (identity 1 of hering_ringpack.h), [limbs][N]"""
    N, j = ring.N, np.arange(ring.N)
    rows = []
    for l, q in enumerate(ring.moduli):
        w = ring.roots(l, backward=div)[(N >> (i + 1)) + (j >> (i + 1))]
        rows.append(np.where((j >> i) & 1 == 1, np.uint64(q) - w, w))
    return np.stack(rows).astype(np.uint64)


def timed(ctx, fn, reps):
    fn()
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def kernels_of(ctx, fn):
    ctx.sync()
    ctx.prof_begin()
    fn()
    prof = ctx.prof_end_bytes()
    out = {}
    for kname, (cnt, kms, kbytes) in prof.items():
        if kname in KERNELS and kms > 0:
            out[kname] = dict(launches=cnt, ms=kms, bytes=kbytes, hbm_fraction=kbytes / (kms * 1e-3) / PEAK_HBM)
    out["total_ms"] = sum(v[1] for v in prof.values())
    return out


def median_rounds(ctx, forms, reps):
    for fn in forms.values():
        fn()
    ctx.sync()
    runs = {name: [] for name in forms}
    for _ in range(3):
        for name, fn in forms.items():
            runs[name].append(timed(ctx, fn, reps))
    return {name: float(np.median(v)) for name, v in runs.items()}


def same(a, b):
    return all(np.array_equal(x.download(), y.download()) for x, y in zip(a, b))


def case_split(ctx, logN, logq, logp, reps, composed_only):
    N, n = 1 << logN, 1 << (logN - 1)
    q, p = O.GenModuli(logN + 1, logq, logp)
    q, p = list(q), list(p)
    L, level = len(q), len(q) - 1
    rng = np.random.default_rng(logN)
    gQ, gP, gs = la.Ring(ctx, N, q), la.Ring(ctx, N, p), la.Ring(ctx, n, q)
    gev = la.Evaluator(gQ, gP)
    k_down, k_up = random_key(rng, gev, q, p, N), random_key(rng, gev, q, p, N)
    xinv0, x0 = la.Poly(gQ, L).upload(xpow2_host(gQ, 0, True)), la.Poly(gQ, L).upload(xpow2_host(gQ, 0, False))
    rQ = gQ.AtLevel(level)
    rp = None if composed_only else R.RingPackingEvaluator({logN: gev, logN - 1: la.Evaluator(gs, la.Ring(ctx, n, p))},
                                                           {(logN, logN - 1): k_down, (logN - 1, logN): k_up})
    res = dict(case=f"split/merge logN {logN}->{logN - 1}", moduli=f"{L}+{len(p)}", reps=reps)
    for B in (1, 32):
        ct = [la.Poly(gQ, L, B).upload(rand_polys(rng, q, N, B)) for _ in range(2)]
        halves = [[la.Poly(gs, L, B).upload(rand_polys(rng, q, n, B)) for _ in range(2)] for _ in range(2)]
        new = lambda g: [la.Poly(g, L, B, zero=False) for _ in range(2)]
        tmp, ce, co, cN = new(gQ), new(gs), new(gs), new(gQ)
        fe, fo, fN = new(gs), new(gs), new(gQ)

        def split_composed():  # ring_packing.go:201-224
            gev.ApplyEvaluationKey(level, ct, k_down, tmp)
            R.SwitchCiphertextRingDegreeNTT(tmp, gQ, ce)
            for t in tmp:
                rQ.MulCoeffsMontgomery(t, xinv0, t)
            R.SwitchCiphertextRingDegreeNTT(tmp, gQ, co)

        def merge_composed():  # :411-420
            R.SwitchCiphertextRingDegreeNTT(halves[0], gQ, cN)
            R.SwitchCiphertextRingDegreeNTT(halves[1], gQ, tmp)
            for t, c in zip(tmp, cN):
                rQ.MulCoeffsMontgomeryThenAdd(t, x0, c)
            gev.ApplyEvaluationKey(level, cN, k_up, cN)

        forms = {"split_composed": split_composed, "merge_composed": merge_composed,
                 "apply_same": lambda: gev.ApplyEvaluationKey(level, ct, k_down, tmp)}
        if not composed_only:
            forms["split_fused"] = lambda: rp.Split(level, ct, fe, fo)
            forms["merge_fused"] = lambda: rp.Merge(level, halves[0], halves[1], fN)
        ms = median_rounds(ctx, forms, reps)
        r = dict(ms=ms)
        if not composed_only:
            split_composed(), merge_composed(), forms["split_fused"](), forms["merge_fused"]()
            r["verified"] = bool(same(fe, ce) and same(fo, co) and same(fN, cN))
            r["split_fused_over_composed"] = ms["split_fused"] / ms["split_composed"]
            r["merge_fused_over_composed"] = ms["merge_fused"] / ms["merge_composed"]
            r["split_over_apply_same"] = ms["split_fused"] / ms["apply_same"]
            r["merge_over_apply_same"] = ms["merge_fused"] / ms["apply_same"]
            r["kernels"] = {"split": kernels_of(ctx, forms["split_fused"]), "merge": kernels_of(ctx, forms["merge_fused"])}
        res[f"batch{B}"] = r
    return res


def galois_keys(rng, gev, q, p, N, galels):
    return R.GaloisKeySet({int(g): random_key(rng, gev, q, p, N) for g in galels})


def small_setup(ctx, logN):
    N = 1 << logN
    q, p = O.GenModuli(logN + 1, [55, 45], [58])
    q, p = list(q), list(p)
    gQ, gP = la.Ring(ctx, N, q), la.Ring(ctx, N, p)
    return N, q, p, gQ, gP, la.Evaluator(gQ, gP), np.random.default_rng(logN)


def case_expand(ctx, reps, composed_only):
    logN = 11
    N, q, p, gQ, gP, gev, rng = small_setup(ctx, logN)
    L, level = len(q), len(q) - 1
    gks = galois_keys(rng, gev, q, p, N, R.GaloisElementsForExpand(2 * N, logN)) if not composed_only else \
        galois_keys(rng, gev, q, p, N, [2 * N // (2 << i) + 1 for i in range(logN)])
    xinv = [la.Poly(gQ, L).upload(xpow2_host(gQ, i, True)) for i in range(logN)]
    rQ = gQ.AtLevel(level)
    Q = int(np.prod([int(x) for x in q], dtype=object))
    NInv = pow(N, -1, Q)
    ct = [la.Poly(gQ, L).upload(rand_polys(rng, q, N, 1)) for _ in range(2)]
    new = lambda: [la.Poly(gQ, L, 1, zero=False) for _ in range(2)]
    out = {}

    def composed():  # ring_packing.go:495-561, one ciphertext per call
        cts = {0: new()}
        for a, b in zip(ct, cts[0]):
            rQ.MulScalarBigint(a, NInv, b)
        tmp = new()
        for i in range(logN):
            n = 1 << i
            galEl = N // n + 1
            gk = gks.GetGaloisKey(galEl)
            for j in range(0, n):
                c0 = cts[j]
                gev.Automorphism(level, c0, galEl, gk, tmp)
                if j + n > 0:
                    c1 = new()
                    for k in range(2):
                        c1[k].CopyLvl(level, c0[k])
                        rQ.Add(c0[k], tmp[k], c0[k])
                        rQ.Sub(c1[k], tmp[k], c1[k])
                        rQ.MulCoeffsMontgomery(c1[k], xinv[i], c1[k])
                    cts[j + n] = c1
                else:
                    for k in range(2):
                        rQ.Add(c0[k], tmp[k], c0[k])
        out["composed"] = cts

    forms = {"expand_composed": composed}
    if not composed_only:
        rp = R.RingPackingEvaluator({logN: gev}, None, None, {logN: gks})

        def fused():
            out["fused"] = rp.Expand(level, ct, 0)
        forms["expand_fused"] = fused
    ms = median_rounds(ctx, forms, reps)
    res = dict(case=f"expand logN {logN} logGap 0", moduli=f"{L}+{len(p)}", reps=reps, ms=ms)
    if not composed_only:
        stack, indices = out["fused"]
        got = [s.download() for s in stack]
        res["verified"] = bool(all(np.array_equal(got[k][e], out["composed"][j][k].download()[0]) for e, j in enumerate(indices) for k in range(2)))
        res["fused_over_composed"] = ms["expand_fused"] / ms["expand_composed"]
        res["kernels"] = kernels_of(ctx, forms["expand_fused"])
    return res


def case_repack(ctx, reps, composed_only):
    logN = 11
    N, q, p, gQ, gP, gev, rng = small_setup(ctx, logN)
    L, level = len(q), len(q) - 1
    galels = [R.GaloisElement(2 * N, 1 << i) for i in range(logN)] + [2 * N - 1]
    gks = galois_keys(rng, gev, q, p, N, galels)
    xpow = [la.Poly(gQ, L).upload(xpow2_host(gQ, i, False)) for i in range(logN)]
    rQ = gQ.AtLevel(level)
    Q = int(np.prod([int(x) for x in q], dtype=object))
    NInv = pow(N, -1, Q)
    src = [[la.Poly(gQ, L).upload(rand_polys(rng, q, N, 1)) for _ in range(2)] for _ in range(N)]
    new = lambda: [la.Poly(gQ, L, 1, zero=False) for _ in range(2)]
    out = {}

    def fresh():  # (the inputs are consumed: every run works on copies, made inside the timed region of both forms)
        cts = {}
        for i, s in enumerate(src):
            c = new()
            for a, b in zip(s, c):
                b.CopyLvl(level, a)
            cts[i] = c
        return cts

    def composed():  # ring_packing.go:668-767 with every index present: the "both" branch throughout
        cts = fresh()
        for c in cts.values():
            for x in c:
                rQ.MulScalarBigint(x, NInv, x)
        tmpa = new()
        for i in range(logN):
            t = 1 << (logN - 1 - i)
            x = xpow[logN - 1 - i]
            galEl = 2 * N - 1 if i == 0 else R.GaloisElement(2 * N, 1 << (i - 1))
            gk = gks.GetGaloisKey(galEl)
            for jx in range(t):
                a, b = cts[jx], cts.pop(jx + t)
                for k in range(2):
                    rQ.MulCoeffsMontgomery(b[k], x, b[k])
                    rQ.Sub(a[k], b[k], tmpa[k])
                    rQ.Add(a[k], b[k], a[k])
                gev.Automorphism(level, tmpa, galEl, gk, tmpa)
                for k in range(2):
                    rQ.Add(a[k], tmpa[k], a[k])
        out["composed"] = cts[0]

    forms = {"repack_composed": composed}
    if not composed_only:
        rp = R.RingPackingEvaluator({logN: gev}, None, {logN: gks}, None)

        def fused():
            out["fused"] = rp.Repack(level, fresh())
        forms["repack_fused"] = fused
    ms = median_rounds(ctx, forms, reps)
    res = dict(case=f"repack of {N} ciphertexts at logN {logN}", moduli=f"{L}+{len(p)}", reps=reps, ms=ms)
    if not composed_only:
        res["verified"] = bool(same(out["fused"], out["composed"]))
        res["fused_over_composed"] = ms["repack_fused"] / ms["repack_composed"]
        res["kernels"] = kernels_of(ctx, forms["repack_fused"])
    return res


def main():
    cases = {"split16": lambda c, a: case_split(c, 16, C5_LOGQ, C5_LOGP, a.reps, a.composed_only),
             "split13": lambda c, a: case_split(c, 13, [55] + [45] * 5, [55] * 2, a.reps, a.composed_only),
             "expand": lambda c, a: case_expand(c, max(1, a.reps // 5), a.composed_only),
             "repack": lambda c, a: case_repack(c, max(1, a.reps // 5), a.composed_only)}
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(cases), action="append")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--composed-only", action="store_true")
    a = ap.parse_args()
    ctx = la.Context(0)
    rc = 0
    for name in a.case or ["split16", "split13", "expand", "repack"]:
        t0 = time.time()
        r = cases[name](ctx, a)
        r["wall_s"] = round(time.time() - t0, 1)
        print(json.dumps(r), flush=True)
        parts = [r] + [v for v in r.values() if isinstance(v, dict)]
        if any(v.get("verified") is False for v in parts):
            rc = 1
        # what must hold by byte count alone: no fused form is slower than the sequence it replaces
        if any(val > 1.0 for v in parts for k, val in v.items() if k.endswith("fused_over_composed")):
            rc = 1
    ctx.sync()
    return rc


if __name__ == "__main__":
    sys.exit(main())
