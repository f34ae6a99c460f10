#!/usr/bin/env python3
"""Times he_complex_to_real and he_real_to_complex (include/hering_bridge.h) against the same-degree he_apply_evaluation_key at
degree N -- the key switch each of them contains, the GadgetProduct with its Add in the epilogue -- at the same batch and level
(every form warmed up first, then three rounds over the forms, the median per form), and reports the two bridge kernels'
bandwidth from the library's own byte accounting.  c2r_over_same / r2c_over_same are the ratios to judge.

    python tools/bridge_bench.py [--shape 16 | 15] [--reps 10]

Shapes: logN 16 <-> 15 with the c5 shape's 25 + 5 moduli at batch 32; logN 15 <-> 14 with 12 + 3 moduli at batch 64.  Every timed
output is checked word for word outside the timed region: the same-degree reference through the oracle's threaded batch key
switch (an automorphism of Galois element 1 is GadgetProduct + Add, core/rlwe/evaluator_automorphism.go:13), the fold and the
unfold (ring/conjugate_invariant.go:3-44) in numpy.  Kernel figures come from he_prof_end_bytes (HIP events around each launch,
the bytes each launcher accounts); the fraction of peak HBM is taken over 8 TB/s.  For a rocprofv3 --kernel-trace --stats run,
pass --no-verify and --reps 3 to keep that run short.  Prints one JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import lattigo_amd as la  # noqa: E402
from lattigo_amd import bridge  # noqa: E402
from oracle import oracle as O  # noqa: E402

PEAK_HBM = 8.0e12
C5_LOGQ = [60] + [40] * 9 + [39] * 3 + [60] * 8 + [56] * 4
C5_LOGP = [61] * 5
SHAPES = {16: (16, C5_LOGQ, C5_LOGP, 32), 15: (15, [55] + [45] * 11, [55] * 3, 64)}


def rand_polys(rng, q, N, B):
    return np.stack([np.stack([rng.integers(0, qi, size=N, dtype=np.uint64) for qi in q]) for _ in range(B)])


def timed(ctx, fn, reps):
    fn()  # warm-up: plans, arena
    ctx.sync()
    ctx.timer_start()
    for _ in range(reps):
        fn()
    return ctx.timer_stop() / reps


def ref_fold(t, q):
    """FoldStandardToConjugateInvariant on [..., L, N]: out[j] = CRed(in[N-1-j] + in[j])"""
    n = t.shape[-1] // 2
    qi = np.array(q, dtype=np.uint64)[:, None]
    s = t[..., ::-1][..., :n] + t[..., :n]
    return np.where(s >= qi, s - qi, s)


def ref_unfold(c):
    return np.concatenate([c, c[..., ::-1]], axis=-1)


def run_shape(ctx, logN, logq, logp, B, reps, verify):
    N, n = 1 << logN, 1 << (logN - 1)
    q, p = O.GenModuli(logN + 1, logq, logp)
    q, p = list(q), list(p)
    L, level = len(q), len(q) - 1
    rng = np.random.default_rng(logN)
    gQ, gP, gci = la.Ring(ctx, N, q), la.Ring(ctx, N, p), la.Ring(ctx, n, q, conjugate_invariant=True)
    gev = la.Evaluator(gQ, gP)
    beta = O.BaseRNSDecompositionVectorSize(L - 1, len(p) - 1)
    kq = np.stack([np.stack([rand_polys(rng, q, N, 1)[0] for _ in range(2)]) for _ in range(beta)])
    kp = np.stack([np.stack([rand_polys(rng, p, N, 1)[0] for _ in range(2)]) for _ in range(beta)])
    gk = gev.NewEvaluationKey(kq, kp)
    sw = bridge.DomainSwitcher(gev, gk, gk)
    big = [rand_polys(rng, q, N, B) for _ in range(2)]
    small = [rand_polys(rng, q, n, B) for _ in range(2)]
    iN = [la.Poly(gQ, L, B).upload(x) for x in big]
    iS = [la.Poly(gci, L, B).upload(x) for x in small]
    oN = [la.Poly(gQ, L, B, zero=False) for _ in range(2)]
    oS = [la.Poly(gci, L, B, zero=False) for _ in range(2)]
    oU = [la.Poly(gQ, L, B, zero=False) for _ in range(2)]
    forms = {
        "apply_same": lambda: gev.ApplyEvaluationKey(level, iN, gk, oN),
        "complex_to_real": lambda: sw.ComplexToReal(iN, oS),
        "real_to_complex": lambda: sw.RealToComplex(iS, oU),
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
    # the kernels of one call of each bridge form, from the library's own accounting
    kern = {}
    for name in ("complex_to_real", "real_to_complex"):
        ctx.sync()
        ctx.prof_begin()
        forms[name]()
        prof = ctx.prof_end_bytes()
        for kname, (cnt, kms, kbytes) in prof.items():
            if kname.startswith("ci_bridge"):
                kern[kname] = dict(launches=cnt, ms=kms, bytes=kbytes, GBs=kbytes / (kms * 1e-3) / 1e9,
                                   hbm_fraction=kbytes / (kms * 1e-3) / PEAK_HBM, share_of_call=kms / sum(v[1] for v in prof.values()))
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
        forms["complex_to_real"]()
        got = np.stack([o.download() for o in oS], axis=1)
        down = ref_fold(same, q)
        good += [bool(np.array_equal(got[b], down[b])) for b in range(B)]
        ctu = np.ascontiguousarray(np.stack([ref_unfold(small[0]), ref_unfold(small[1])], axis=1))
        up = oev.BatchOp("rotate", ctu, key=ok, gal=1)
        forms["real_to_complex"]()
        got = np.stack([o.download() for o in oU], axis=1)
        good += [bool(np.array_equal(got[b], up[b])) for b in range(B)]
        verified = f"{sum(good)}/{len(good)}"
        verify_s = time.time() - t0
    return dict(shape=f"logN {logN}<->{logN - 1}", moduli=f"{L}+{len(p)}", batch=B, level=level, reps=reps, ms=ms, ms_rounds=runs,
                c2r_over_same=ms["complex_to_real"] / ms["apply_same"], r2c_over_same=ms["real_to_complex"] / ms["apply_same"],
                map_working_set_MiB=2.0 * B * L * (N + n) * 8 / 2**20, kernels=kern,
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
