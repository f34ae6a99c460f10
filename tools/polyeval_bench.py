#!/usr/bin/env python3
"""Times a polynomial evaluation whose baby steps go through he_polyeval_leaves (include/hering_polyeval.h; the leaf-group kernel at
G = 1, 2, 4 baby steps per launch, tests/drivers/polyeval_native.py) against the driver of tests/drivers/polyeval.py, which makes one
scalar launch per constant and per (term, component) -- the same power basis and giant steps, composed of the operator entries, on
the same handles and words.

    python tools/polyeval_bench.py [--shape c5 | 14] [--batches 1,16,32]

Shapes: the EvalMod polynomial of the bootstrap shape of tools/bootstrap_c5_shape.py (logN 16, 25 + 5 moduli, input at level 20 and
scale 2^60, an even Chebyshev polynomial of degree 30) and logN 14 with 8 + 2 moduli at degree 31 (Chebyshev, no parity).  The
relinearization key and the input are synthetic uniform words and the coefficients random (throughput does not depend on their
values; tests/test_gpu_polyeval.py holds the words against the reference).  Every leg (driver, g1, g2, g4) runs in a fresh process
of its own under `timeout`, three of them per leg, the legs alternating; a process warms a batch up, sizes a window of about 0.3 s
from three calls, then times that many calls between device events (he_timer_*).  The figure of a leg is the median of its three
processes.  Every process hashes its outputs: the parent checks that all legs agree.  The last process of each leg also profiles one
call per batch (he_prof_end_bytes) for the launch count, the device time, and the baby steps' share: the element-wise launches of
the driver's baby steps, or the leaf-group kernel's launches, time, bytes (the launcher's own accounting) and fraction of 8 TB/s.
Prints one JSON line per shape.

    python tools/polyeval_bench.py --leg g2 --shape c5 --batches 1,16     (one process of one leg: what the parent starts)"""
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
# (logN, log2 of the moduli of Q, of P, input level, log2 of the scale, degree, parity)
SHAPES = {"c5": (16, [60] + [40] * 9 + [39] * 3 + [60] * 8 + [56] * 4, [61] * 5, 20, 60, 30, "even"),
          "14": (14, [55] + [45] * 7, [55] * 2, 7, 45, 31, "both")}


def run_leg(leg, shape, batches, profile):
    from fractions import Fraction

    import lattigo_amd as la
    from bench import uniform
    from drivers import polyeval as PE
    from drivers import schemes as S
    from drivers.polyeval_native import NativeLeaves
    from bootstrap_c5_shape import gen_primes  # (tools/ is the script's directory)

    logN, logq, logp, level, logscale, degree, parity = SHAPES[shape]
    N, nth = 1 << logN, 2 << logN
    taken = set()
    q, p = gen_primes(logq, nth, taken), gen_primes(logp, nth, taken)
    top, LP = len(q) - 1, len(p)
    ctx = la.Context(0)
    rq, rp = la.Ring(ctx, N, q), la.Ring(ctx, N, p)
    ev = la.Evaluator(rq, rp)
    rng = np.random.Generator(np.random.PCG64(0x90E7 + logN))
    beta = (top + 1 + LP - 1) // LP
    rlk = ev.NewEvaluationKey(uniform(rng, q, N, (beta, 2)), uniform(rng, p, N, (beta, 2)))
    ce = S.CKKSCiphertextEvaluator(ev, rlk)
    scale = Fraction(1 << logscale)
    coeffs = [PE._cpair(float(c)) if (parity == "both" or k % 2 == 0) else None for k, c in enumerate(rng.uniform(-1, 1, size=degree + 1))]

    def pol():
        x = PE.Polynomial(list(coeffs), Basis="Chebyshev")
        x.IsEven, x.IsOdd = parity in ("both", "even"), parity in ("both", "odd")
        return x

    pe = PE.PolynomialEvaluator(ce) if leg == "driver" else NativeLeaves(ce, rq, int(leg[1:]))
    out = dict(leg=leg, shape=shape, logN=logN, moduli=f"{top + 1}+{LP}", level=level, degree=degree, parity=parity, ms={}, reps={}, digest={},
               kernels={})
    for B in batches:
        brng = np.random.Generator(np.random.PCG64(1000 * logN + B))  # the same words in every process and leg
        ct = S.Ciphertext([la.Poly(rq, level + 1, B).upload(uniform(brng, q[: level + 1], N, (B,))) for _ in range(2)], level, scale)
        call = lambda: pe.Evaluate(ct, pol(), scale)
        call()  # warm-up: plans, the handle, arena, buffer cache
        res = call()
        ctx.sync()
        ctx.timer_start()
        for _ in range(3):
            call()
        reps = int(min(max(WINDOW_MS / (ctx.timer_stop() / 3), 5), 2000))
        ctx.timer_start()
        for _ in range(reps):
            res = call()
        out["ms"][B] = ctx.timer_stop() / reps
        out["reps"][B] = reps
        h = hashlib.sha256()
        for x in res.Value:
            h.update(x.download()[:, : res.level + 1].tobytes())
        out["digest"][B] = h.hexdigest()[:16]
        if leg != "driver":
            out["baby_steps"] = len(pe.planned.leaves)
            out["terms"] = sum(len(f["words"]) for f in pe.planned.leaves)
        if profile:
            ctx.sync()
            ctx.prof_begin()
            call()
            prof = ctx.prof_end_bytes()
            total = sum(v[1] for v in prof.values())
            k = dict(launches=sum(v[0] for v in prof.values()), device_ms=round(total, 4))
            for name in ("ew", "poly_leaf_group"):
                if name in prof:
                    c, ms, by = prof[name]
                    k[name] = dict(launches=c, ms=round(ms, 4), share=round(ms / total, 4), bytes=by, GBs=by / (ms * 1e-3) / 1e9 if ms else 0.0,
                                   hbm_fraction=by / (ms * 1e-3) / PEAK_HBM if ms else 0.0)
            out["kernels"][B] = k
        del ct, res
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
        first = runs["g1"][0]
        res = dict(shape=s, logN=first["logN"], moduli=first["moduli"], level=first["level"], degree=first["degree"], parity=first["parity"],
                   baby_steps=first.get("baby_steps"), scalars=first.get("terms"), processes=a.processes, batches={})
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
