#!/usr/bin/env python3
"""Times he_lintrans_evaluate_many (include/hering_lintrans.h) against the driver of tests/drivers/lintrans.py -- the same product
driven through the rlwe.EvaluatorProvider operators one call at a time -- on the same handles and words, at every grouping of the
giant steps (he_lintrans_set_group: G = 1, 2, 4).

    python tools/lintrans_bench.py [--shape c5 | 14] [--batches 1,16,32]

Shapes: the first CoeffsToSlots factor of the bootstrap shape of tools/bootstrap_c5_shape.py (logN 16, 25 + 5 moduli, the 16
distinct diagonals {j 2^11 mod 2^15 : |j| < 16}, logBSGSRatio 1) and logN 14 with 8 + 2 moduli (the same diagonal structure at stride 2^9).  Keys,
diagonals and the input are synthetic uniform words (throughput does not depend on their values; tests/test_gpu_lintrans.py holds
the words against the reference).  Every leg (driver, g1, g2, g4) runs in a fresh process of its own under `timeout`, three of
them per leg, the legs alternating; a process warms a batch up, sizes a window of about 0.3 s from three calls, then times that
many calls between device events (he_timer_*).  The figure of a leg is the median of its three processes.  Every process hashes
its outputs: the parent checks that all legs agree.  The last process of each leg also profiles one call per batch
(he_prof_end_bytes) for the launch count, the device time, and the multiply-accumulate kernel's time, bytes (the launcher's own
accounting) and fraction of 8 TB/s.  Prints one JSON line per shape.

    python tools/lintrans_bench.py --leg g2 --shape c5 --batches 1,16     (one process of one leg: what the parent starts)"""
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
WINDOW_MS = 300.0
LEGS = ("driver", "g1", "g2", "g4")
# (logN, log2 of the moduli of Q, of P, radix-2 layers merged in the factor, log2 of its stride)
SHAPES = {"c5": (16, [60] + [40] * 9 + [39] * 3 + [60] * 8 + [56] * 4, [61] * 5, 4, 11), "14": (14, [55] + [45] * 7, [55] * 2, 4, 9)}


def run_leg(leg, shape, batches, profile):
    import math

    import lattigo_amd as la
    from bench import uniform
    from drivers import lintrans as LT
    from lattigo_amd import lintrans as NL
    from lattigo_amd import rlwe as R
    from bootstrap_c5_shape import gen_primes  # (tools/ is the script's directory)

    logN, logq, logp, k, s = SHAPES[shape]
    N, n, nth = 1 << logN, 1 << (logN - 1), 2 << logN
    taken = set()
    q, p = gen_primes(logq, nth, taken), gen_primes(logp, nth, taken)
    top, LP = len(q) - 1, len(p)
    ctx = la.Context(0)
    rq, rp = la.Ring(ctx, N, q), la.Ring(ctx, N, p)
    ev = la.Evaluator(rq, rp)
    rng = np.random.Generator(np.random.PCG64(0x11A7 + logN))
    beta = (top + 1 + LP - 1) // LP
    kq, kp = uniform(rng, q, N, (beta, 2)), uniform(rng, p, N, (beta, 2))  # one synthetic key image, uploaded per key
    dq, dp = uniform(rng, q, N), uniform(rng, p, N)
    diags = sorted({(j << s) % n for j in range(-(1 << k) + 1, 1 << k)})
    N1 = LT.FindBestBSGSRatio(diags, n, 1)
    _, r1, r2 = LT.BSGSIndex(diags, n, N1)
    gks = R.GaloisKeySet()
    for r in sorted(set(r1) | set(r2)):
        if r:
            gks.keys[R.GaloisElement(nth, r)] = ev.NewEvaluationKey(kq, kp)
    vec = {d: (la.Poly(rq, top + 1).upload(dq), la.Poly(rp, LP).upload(dp)) for d in diags}
    if leg == "driver":
        lt, le = LT.LinearTransformation(vec, top, LP - 1, n, N1), LT.LinTransEvaluator(ev, gks)
    else:
        lt, le = NL.LinearTransformation(ev, vec, top, LP - 1, (0, int(math.log2(n))), N1), NL.Evaluator(ev, gks)
        lt.SetGroup(int(leg[1:]))
    out = dict(leg=leg, shape=shape, logN=logN, moduli=f"{top + 1}+{LP}", diagonals=len(diags), N1=N1, giants=len(r1), babies=len(r2),
               ms={}, reps={}, digest={}, kernels={})
    for B in batches:
        brng = np.random.Generator(np.random.PCG64(1000 * logN + B))  # the same words in every process and leg
        ct = [la.Poly(rq, top + 1, B).upload(uniform(brng, q, N, (B,))) for _ in range(2)]
        o = [la.Poly(rq, top + 1, B, zero=False) for _ in range(2)]
        call = lambda: le.EvaluateMany(top, ct, [lt], [o])
        call()  # warm-up: plans, index tables, arena, buffer cache
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
            mac = {}
            for name in ("diag_mac", "diag_mac_group"):
                if name in prof:
                    c, ms, by = prof[name]
                    mac[name] = dict(launches=c, ms=round(ms, 4), share=round(ms / total, 4), bytes=by, GBs=by / (ms * 1e-3) / 1e9,
                                     hbm_fraction=by / (ms * 1e-3) / PEAK_HBM)
            out["kernels"][B] = dict(launches=sum(v[0] for v in prof.values()), device_ms=round(total, 4), mac=mac)
        del ct, o
    ctx.sync()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), action="append")
    ap.add_argument("--batches", default="1,16,32")
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds one process of one leg may take")
    a = ap.parse_args()
    batches = [int(x) for x in a.batches.split(",")]
    if a.leg:  # one process of one leg
        print(json.dumps(run_leg(a.leg, (a.shape or ["c5"])[0], batches, a.profile)), flush=True)
        return 0
    rc = 0
    for s in a.shape or ["c5", "14"]:
        runs = {leg: [] for leg in LEGS}
        for i in range(a.processes):  # the legs alternate: none owes its figure to its place in the order
            for leg in LEGS:
                cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--leg", leg, "--shape", s,
                       "--batches", a.batches]
                if i == a.processes - 1:
                    cmd.append("--profile")
                r = subprocess.run(cmd, capture_output=True, text=True)
                if r.returncode != 0:  # (a process that failed, faulted or ran out of time ends the measurement: nothing more is started)
                    print(f"leg {leg} of shape {s} ended with status {r.returncode}\n" + r.stdout + r.stderr, file=sys.stderr)
                    return 1
                runs[leg].append(json.loads(r.stdout.strip().splitlines()[-1]))
                print(f"shape {s} process {i + 1}/{a.processes} leg {leg}: {runs[leg][-1]['ms']}", file=sys.stderr, flush=True)
        first = runs["driver"][0]
        res = dict(shape=s, logN=first["logN"], moduli=first["moduli"], diagonals=first["diagonals"], N1=first["N1"], giants=first["giants"],
                   babies=first["babies"], processes=a.processes, batches={})
        for B in batches:
            key = str(B)
            ms = {leg: float(np.median([r["ms"][key] for r in runs[leg]])) for leg in LEGS}
            same = len({r["digest"][key] for leg in LEGS for r in runs[leg]}) == 1
            rc |= 0 if same else 1
            drv = [r["ms"][key] for r in runs["driver"]]
            res["batches"][B] = dict(ms=ms, ms_processes={leg: [r["ms"][key] for r in runs[leg]] for leg in LEGS},
                                     driver_spread=(max(drv) - min(drv)) / ms["driver"],
                                     driver_over={leg: ms["driver"] / ms[leg] for leg in LEGS[1:]}, all_legs_equal=same,
                                     kernels={leg: runs[leg][-1]["kernels"].get(key) for leg in LEGS})
        print(json.dumps(res), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
