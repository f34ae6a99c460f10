#!/usr/bin/env python3
"""Times the device samplers (lattigo_amd.sampling, include/hering_sampler.h) on the system source at the headline shape: logN 15,
12 + 3 moduli, batch 1 and 64.

    python tools/sampler_bench.py [--rounds 5]

Per sampler and batch: the wall-clock time of one call (median over `--rounds` calls after a warm-up; a call returns with the
device drained), the device time of its launches and their count from a separate profiled call (he_prof_end), and the time
os.getrandom takes for the bytes the call consumes -- the floor that the host source sets.  wall - device is what the host spends
fetching, staging and wiping.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()

    import lattigo_amd as la
    from lattigo_amd import sampling
    from tests.rlwe_fixtures import downstream_primes

    logN, nq, npp = 15, 12, 3
    pr = downstream_primes(55, 2 << logN, nq + npp)
    ctx = la.Context(0)
    rq, rp = la.Ring(ctx, 1 << logN, pr[:nq]), la.Ring(ctx, 1 << logN, pr[nq:])
    prng = sampling.PRNG()
    out = {"logN": logN, "limbs": [nq, npp], "rounds": a.rounds, "cases": []}
    for batch in (1, 64):
        q, p = rq.NewPoly(batch), rp.NewPoly(batch)
        calls = {
            "uniform_qp": lambda: sampling.UniformSampler(prng, rq, rp).Read((q, p)),
            "uniform_q": lambda: sampling.UniformSampler(prng, rq).Read(q),
            "gaussian": lambda: sampling.GaussianSampler(prng, rq, 3.2, 19.2, False).Read(q),
            "ternary_2_3": lambda: sampling.TernarySampler(prng, rq, 2 / 3, True).Read(q),
            "ternary_half": lambda: sampling.TernarySampler(prng, rq, 0.5, True).Read(q),
        }
        for name, call in calls.items():
            call()
            walls, consumed = [], 0
            for _ in range(a.rounds):
                at = prng.Position()
                t0 = time.perf_counter()
                call()
                walls.append((time.perf_counter() - t0) * 1e3)
                consumed = prng.Position() - at
            ctx.prof_begin()
            call()
            prof = ctx.prof_end()
            t0 = time.perf_counter()
            left = consumed
            while left > 0:
                left -= len(os.getrandom(min(left, 1 << 24)))
            source_ms = (time.perf_counter() - t0) * 1e3
            out["cases"].append({"sampler": name, "batch": batch, "wall_ms": round(statistics.median(walls), 3),
                                 "device_ms": round(sum(v[1] for v in prof.values()), 3), "launches": sum(v[0] for v in prof.values()),
                                 "kernels": {k: [v[0], round(v[1], 3)] for k, v in prof.items()}, "bytes_consumed": consumed,
                                 "getrandom_ms": round(source_ms, 3)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
