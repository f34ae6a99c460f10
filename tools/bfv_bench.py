#!/usr/bin/env python3
"""Times he_bfv_mul_relin (include/hering_bfv.h) against the driver sequence of tests/drivers/bgv.py -- the same multiplication
driven through the ring operators one call at a time -- on the same words, and against he_bgv_mul_relin on the same shape for
scale.

    python tools/bfv_bench.py [--shape 15 | 13] [--batches 1,16,64]

Shapes: the headline shape (logN 15, 12 + 3 moduli, t = 65537; QMul: as many 61-bit moduli as levelQMul asks for) and logN 13
(6 + 2 moduli).  Every leg (native, driver, bgv) runs in a fresh process of its own, three of them per leg, one after the other;
a process warms a batch up, sizes a window of about 0.3 s from three calls, then times that many calls between device events
(he_timer_*).  The figure of a leg is the median of its three processes.  The native and the driver processes hash their
outputs: the parent checks that they agree (tests/test_gpu_bfv.py holds both against the reference).  The last process of the
native and of the driver leg also profiles one call per batch (he_prof_end_bytes: HIP events around each launch, the bytes each
launcher accounts) for the launch counts, the per-kernel split and the quantize kernel's achieved bytes/s; the fraction of peak
HBM is over 8 TB/s.  Prints one JSON line per shape.

    python tools/bfv_bench.py --leg native --shape 15 --batches 1,16     (one process of one leg: what the parent starts)"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_HBM = 8.0e12
T = 65537
SHAPES = {15: ([55] + [45] * 11, [55] * 3), 13: ([55] + [45] * 5, [55] * 2)}
WINDOW_MS = 300.0  # a timed window: long enough that the clock and the scheduler do not decide the figure
LEGS = ("native", "driver", "bgv")


def rand_polys(rng, q, N, B):
    return np.stack([np.stack([rng.integers(0, qi, size=N, dtype=np.uint64) for qi in q]) for _ in range(B)])


def run_leg(leg, logN, batches, profile):
    import lattigo_amd as la
    from drivers import bgv as DRV
    from lattigo_amd import bfv as BFV
    from oracle import oracle as O
    from tests.rlwe_fixtures import downstream_primes

    logq, logp = SHAPES[logN]
    N = 1 << logN
    q, p = O.GenModuli(logN + 1, logq, logp)
    q, p = [int(x) for x in q], [int(x) for x in p]
    L, level = len(q), len(q) - 1
    bits = sum(x.bit_length() for x in q)
    Q = 1
    for x in q:
        Q *= x
    nm = -(-(Q.bit_length() + logN) // 61)
    qm = downstream_primes(61, 2 * N, nm, set(q) | set(p))
    rng = np.random.default_rng(logN)
    ctx = la.Context(0)
    gQ, gP, gM = la.Ring(ctx, N, q), la.Ring(ctx, N, p), la.Ring(ctx, N, qm)
    gev = la.Evaluator(gQ, gP)
    beta = O.BaseRNSDecompositionVectorSize(L - 1, len(p) - 1)
    kq = np.stack([np.stack([rand_polys(rng, q, N, 1)[0] for _ in range(2)]) for _ in range(beta)])
    kp = np.stack([np.stack([rand_polys(rng, p, N, 1)[0] for _ in range(2)]) for _ in range(beta)])
    gk = gev.NewEvaluationKey(kq, kp)
    ev = {"native": BFV.ScaleInvariantEvaluator, "driver": DRV.ScaleInvariantEvaluator}.get(leg)
    ev = ev(gev, gM, T) if ev else None
    out = dict(leg=leg, logN=logN, moduli=f"{L}+{len(p)}", qmul=nm, q_bits=bits, ms={}, reps={}, digest={}, kernels={})
    for B in batches:
        brng = np.random.default_rng(1000 * logN + B)  # the same words in every process and leg
        a = [la.Poly(gQ, L, B).upload(rand_polys(brng, q, N, B)) for _ in range(2)]
        b = [la.Poly(gQ, L, B).upload(rand_polys(brng, q, N, B)) for _ in range(2)]
        o = [la.Poly(gQ, L, B, zero=False) for _ in range(2)]
        if leg == "bgv":
            call = lambda: gev.BGVMulRelin(level, T, a, b, gk, o)
        else:
            call = lambda: ev.MulRelinScaleInvariant(level, a, b, gk, o)
        call()  # warm-up: plans, arena, buffer cache
        call()
        ctx.sync()
        ctx.timer_start()
        for _ in range(3):
            call()
        reps = int(min(max(WINDOW_MS / (ctx.timer_stop() / 3), 5), 2000))
        ctx.timer_start()
        for _ in range(reps):
            call()
        out["ms"][B] = ctx.timer_stop() / reps
        out["reps"][B] = reps
        h = hashlib.sha256()
        for x in o:
            h.update(x.download().tobytes())
        out["digest"][B] = h.hexdigest()[:16]
        if profile:
            ctx.sync()
            ctx.prof_begin()
            call()
            prof = ctx.prof_end_bytes()
            total = sum(v[1] for v in prof.values())
            k = {name: dict(launches=c, ms=round(ms, 4), share=round(ms / total, 4)) for name, (c, ms, _) in sorted(prof.items(), key=lambda kv: -kv[1][1])}
            if "bfv_quantize" in prof:
                c, ms, by = prof["bfv_quantize"]
                k["bfv_quantize"].update(bytes=by, GBs=by / (ms * 1e-3) / 1e9, hbm_fraction=by / (ms * 1e-3) / PEAK_HBM)
            out["kernels"][B] = dict(launches=sum(v[0] for v in prof.values()), device_ms=round(total, 4), by_kernel=k)
        del a, b, o
    ctx.sync()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, choices=sorted(SHAPES), action="append")
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--processes", type=int, default=3)
    a = ap.parse_args()
    batches = [int(x) for x in a.batches.split(",")]
    if a.leg:  # one process of one leg
        print(json.dumps(run_leg(a.leg, (a.shape or [15])[0], batches, a.profile)), flush=True)
        return 0
    rc = 0
    for s in a.shape or sorted(SHAPES, reverse=True):
        runs = {leg: [] for leg in LEGS}
        for i in range(a.processes):  # the legs alternate: none owes its figure to its place in the order
            for leg in LEGS:
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--shape", str(s), "--batches", a.batches]
                if leg != "bgv" and i == a.processes - 1:
                    cmd.append("--profile")
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                if r.returncode != 0:
                    print(r.stdout + r.stderr, file=sys.stderr)
                    return 1
                runs[leg].append(json.loads(r.stdout.strip().splitlines()[-1]))
        res = dict(shape=f"logN {s}", moduli=runs["native"][0]["moduli"], qmul=runs["native"][0]["qmul"], t=T, processes=a.processes, batches={})
        for B in batches:
            key = str(B)
            ms = {leg: float(np.median([r["ms"][key] for r in runs[leg]])) for leg in LEGS}
            same = len({r["digest"][key] for leg in ("native", "driver") for r in runs[leg]}) == 1
            rc |= 0 if same else 1
            res["batches"][B] = dict(ms=ms, ms_processes={leg: [r["ms"][key] for r in runs[leg]] for leg in LEGS},
                                     driver_over_native=ms["driver"] / ms["native"], native_over_bgv=ms["native"] / ms["bgv"],
                                     native_equals_driver=same, native_kernels=runs["native"][-1]["kernels"].get(key),
                                     driver_launches=(runs["driver"][-1]["kernels"].get(key) or {}).get("launches"))
        print(json.dumps(res), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
