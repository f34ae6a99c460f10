#!/usr/bin/env python3
"""Times he_apply_evaluation_key (include/hering_ringswitch.h) in its three degree forms against he_gadget_product at degree N, at
the same batch and level (every form warmed up first, then three rounds over the forms, the median per form), and reports the
fold / replicate kernels' bandwidth from the library's own byte accounting.  The key switch a degree-changing call contains is
the same-degree call (the GadgetProduct with its Add in the epilogue): down_over_same / up_over_same are the ratios to judge.

    python tools/ringswitch_bench.py [--shape 16 | 15] [--reps 10]

Shapes: logN 16 <-> 15 with the c5 shape's 25 + 5 moduli at batch 32; logN 15 <-> 14 with 12 + 3 moduli at batch 64.  Every timed
output is checked word for word against the oracle outside the timed region (the same-degree reference through the oracle's
threaded batch key switch -- an automorphism of Galois element 1 is GadgetProduct + Add, core/rlwe/evaluator_automorphism.go:13 --,
the degree maps through its INTT / NTT).  Kernel figures come from he_prof_end_bytes (HIP events around each launch, the bytes each
launcher accounts); the fraction of peak HBM is taken over 8 TB/s.  For a rocprofv3 --kernel-trace --stats run, pass --no-verify
and --reps 3 to keep that run short.  Prints one JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import lattigo_amd as la  # noqa: E402
from oracle import oracle as O  # noqa: E402

PEAK_HBM = 8.0e12
C5_LOGQ = [60] + [40] * 9 + [39] * 3 + [60] * 8 + [56] * 4
C5_LOGP = [61] * 5
SHAPES = {16: (16, 15, C5_LOGQ, C5_LOGP, 32), 15: (15, 14, [55] + [45] * 11, [55] * 3, 64)}


def rand_polys(rng, q, N, B):
    return np.stack([np.stack([rng.integers(0, qi, size=N, dtype=np.uint64) for qi in q]) for _ in range(B)])


def timed(ctx, fn, reps):
    fn()  # warm-up: plans, arena
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def ref_down(t, q, N, gap):
    """SwitchCiphertextRingDegreeNTT N -> N / gap of [B][2][L][N] (core/rlwe/element.go:260-279)"""
    big, small = O.Ring(N, q), O.Ring(N // gap, q)
    return np.stack([np.stack([small.NTT(big.INTT(t[b, k])[:, ::gap].copy()) for k in range(2)]) for b in range(t.shape[0])])


def run_shape(ctx, logN, logn, logq, logp, B, reps, verify):
    N, n, gap = 1 << logN, 1 << logn, 1 << (logN - logn)
    q, p = O.GenModuli(logN + 1, logq, logp)
    q, p = list(q), list(p)
    L, level = len(q), len(q) - 1
    rng = np.random.default_rng(logN)
    gQ, gP, gs = la.Ring(ctx, N, q), la.Ring(ctx, N, p), la.Ring(ctx, n, q)
    gev = la.Evaluator(gQ, gP)
    beta = O.BaseRNSDecompositionVectorSize(L - 1, len(p) - 1)
    kq = np.stack([np.stack([rand_polys(rng, q, N, 1)[0] for _ in range(2)]) for _ in range(beta)])
    kp = np.stack([np.stack([rand_polys(rng, p, N, 1)[0] for _ in range(2)]) for _ in range(beta)])
    gk = gev.NewEvaluationKey(kq, kp)
    big = [rand_polys(rng, q, N, B) for _ in range(2)]
    small = [rand_polys(rng, q, n, B) for _ in range(2)]
    iN = [la.Poly(gQ, L, B).upload(x) for x in big]
    iS = [la.Poly(gs, L, B).upload(x) for x in small]
    oN = [la.Poly(gQ, L, B, zero=False) for _ in range(2)]
    oS = [la.Poly(gs, L, B, zero=False) for _ in range(2)]
    oU = [la.Poly(gQ, L, B, zero=False) for _ in range(2)]
    forms = {
        "gadget_product": lambda: gev.GadgetProduct(level, iN[1], gk, oN),
        "apply_same": lambda: gev.ApplyEvaluationKey(level, iN, gk, oN),
        "apply_down": lambda: gev.ApplyEvaluationKey(level, iN, gk, oS),
        "apply_up": lambda: gev.ApplyEvaluationKey(level, iS, gk, oU),
    }
    for fn in forms.values():  # every form warmed up (plans, arena) before any is timed
        fn()
    ctx.sync()
    # three rounds over the forms, the median per form: no form owes its figure to its place in the order
    runs = {name: [] for name in forms}
    for _ in range(3):
        for name, fn in forms.items():
            runs[name].append(timed(ctx, fn, reps))
    ms = {name: float(np.median(v)) for name, v in runs.items()}
    # the kernels of one call of each degree-changing form, from the library's own accounting
    kern = {}
    for name in ("apply_down", "apply_up"):
        ctx.sync()
        ctx.prof_begin()
        forms[name]()
        prof = ctx.prof_end_bytes()
        for kname, (cnt, kms, kbytes) in prof.items():
            if kname.startswith("ring_degree"):
                kern[kname] = dict(launches=cnt, ms=kms, bytes=kbytes, GBs=kbytes / (kms * 1e-3) / 1e9,
                                   hbm_fraction=kbytes / (kms * 1e-3) / PEAK_HBM)
        kern[name + "_total_ms"] = sum(v[1] for v in prof.values())
    verified = None
    if verify:
        t0 = time.time()
        oQ, oP = O.Ring(N, q), O.Ring(N, p)
        oev = O.Evaluator(oQ, oP)
        ok = O.EvaluationKey(kq, kp)
        ct = np.ascontiguousarray(np.stack([big[0], big[1]], axis=1))  # [B][2][L][N]
        same = oev.BatchOp("rotate", ct, key=ok, gal=1)
        forms["apply_same"]()
        got = np.stack([o.download() for o in oN], axis=1)
        good = [bool(np.array_equal(got[b], same[b])) for b in range(B)]
        forms["gadget_product"]()
        gp = np.stack([o.download() for o in oN], axis=1)
        sub = O.Ring(N, q)
        good += [bool(np.array_equal(gp[b, 1], same[b, 1]) and np.array_equal(sub.binop("Add", big[0][b], gp[b, 0]), same[b, 0]))
                 for b in range(B)]
        forms["apply_down"]()
        got = np.stack([o.download() for o in oS], axis=1)
        down = ref_down(same, q, N, gap)
        good += [bool(np.array_equal(got[b], down[b])) for b in range(B)]
        ctu = np.ascontiguousarray(np.stack([np.repeat(small[0], gap, axis=2), np.repeat(small[1], gap, axis=2)], axis=1))
        up = oev.BatchOp("rotate", ctu, key=ok, gal=1)
        forms["apply_up"]()
        got = np.stack([o.download() for o in oU], axis=1)
        good += [bool(np.array_equal(got[b], up[b])) for b in range(B)]
        verified = f"{sum(good)}/{len(good)}"
        verify_s = time.time() - t0
    fold_bytes = 2.0 * B * L * (N + n) * 8
    # the key switch a degree-changing call contains is the same-degree call (GadgetProduct with the Add in its epilogue)
    return dict(shape=f"logN {logN}<->{logn}", moduli=f"{L}+{len(p)}", batch=B, level=level, reps=reps, ms=ms, ms_rounds=runs,
                down_over_same=ms["apply_down"] / ms["apply_same"], up_over_same=ms["apply_up"] / ms["apply_same"],
                down_over_gp=ms["apply_down"] / ms["gadget_product"], up_over_gp=ms["apply_up"] / ms["gadget_product"],
                same_over_gp=ms["apply_same"] / ms["gadget_product"], fold_working_set_MiB=fold_bytes / 2**20, kernels=kern,
                verified=verified, **({"verify_s": round(verify_s, 1)} if verify else {}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, choices=sorted(SHAPES), action="append")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-verify", action="store_true")
    a = ap.parse_args()
    ctx = la.Context(0)
    rc = 0
    for s in a.shape or sorted(SHAPES, reverse=True):
        r = run_shape(ctx, *SHAPES[s], a.reps, not a.no_verify)
        print(json.dumps(r), flush=True)
        if r["verified"] is not None and r["verified"].split("/")[0] != r["verified"].split("/")[1]:
            rc = 1
    ctx.sync()
    return rc


if __name__ == "__main__":
    sys.exit(main())
