#!/usr/bin/env python3
"""Times he_blind_rotate_core (include/hering_blindrot.h) at the reference's own test shape -- N_BR = 1024, Q = 0x7fff801,
BaseTwoDecomposition 7, no special prime, N_LWE = 512 (core/rgsw/blindrot/blindrot_test.go:53-71) -- two ways:

  per_entry  HERING_NO_BLINDROT_BATCH=1: every batch entry runs the reference's own order through the launches of
             he_rgsw_external_product and he_automorphism_ct, the entry points the library had before.  The baseline.
  batched    the merged rounds: one he_automorphism_ct_select launch and one he_rgsw_external_product_select launch per round
             over the whole batch

    python tools/blindrot_bench.py [--batch 1 16 128] [--seconds 0.5] [--rounds 3]

Every configuration (batch, leg) runs in a process of its own, legs alternating, `--rounds` rounds, and the median is reported
(the switch is read once per process).  A child warms its shape up, sizes its repetition count to fill `--seconds` (at least
two calls), times that many calls between device events and counts the launches of one call with the kernel profiler in a
separate, untimed pass.  The two legs' outputs on the same seeded inputs are compared word for word (a digest).  Prints one
JSON line per child and one per batch with blind rotations per second; exit status non-zero when a digest differs."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOGN, Q, PW2, N_LWE = 10, 0x7FFF801, 7, 512
LEGS = ("per_entry", "batched")


def child(batch, leg, seconds, n_lwe):
    import lattigo_amd as la
    from lattigo_amd import blindrot as B
    from lattigo_amd import rgsw as G

    N = 1 << LOGN
    rng = np.random.default_rng(20261018)
    ctx = la.Context(0)
    gQ = la.Ring(ctx, N, [Q])
    gev = G.Evaluator(gQ, None)
    nj = [(Q.bit_length() + PW2 - 1) // PW2]
    D = nj[0]
    key = lambda: gev.NewEvaluationKey(rng.integers(0, Q, size=(D, 2, 1, N), dtype=np.uint64), None, PW2, nj)
    brk = [G.Ciphertext(key(), key()) for _ in range(n_lwe)]
    BRK = B.MemBlindRotationEvaluationKeySet(gev, brk, {g: key() for g in B.GaloisElements(N)})
    rows = (rng.integers(0, N, size=(batch, n_lwe)) * 2 + 1).astype(np.uint64)
    start = rng.integers(0, Q, size=(2, batch, 1, N), dtype=np.uint64)
    fresh = [la.Poly(gQ, 1, batch).upload(start[k]) for k in range(2)]
    acc = [la.Poly(gQ, 1, batch) for _ in range(2)]
    ev = B.Evaluator(gev, gQ)

    def call():
        ev.BlindRotateCore(rows, acc, BRK)

    [a.CopyLvl(0, f) for a, f in zip(acc, fresh)]
    call()
    ctx.sync()
    digest = hashlib.sha256(b"".join(a.download().tobytes() for a in acc)).hexdigest()[:16]
    ctx.prof_begin()
    call()
    prof = ctx.prof_end()
    launches = int(sum(n for n, _ in prof.values()))
    ctx.sync()
    ctx.timer_start()
    call()
    per = max(ctx.timer_stop(), 1e-3)  # ms
    reps = int(min(max(seconds * 1e3 / per, 2), 2000))
    ctx.timer_start()
    for _ in range(reps):
        call()
    ms = ctx.timer_stop() / reps
    print(json.dumps(dict(batch=batch, leg=leg, n_lwe=n_lwe, ms=ms, reps=reps, launches=launches, rotations_per_s=batch / (ms * 1e-3),
                          rounds=len(B.Rounds(LOGN, rows)), digest=digest)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", nargs="+", type=int, default=[1, 16, 128])
    ap.add_argument("--leg", choices=LEGS, help="run one configuration in this process (what the parent starts)")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n-lwe", type=int, default=N_LWE)
    a = ap.parse_args()
    if a.leg:
        child(a.batch[0], a.leg, a.seconds, a.n_lwe)
        return 0
    bad = 0
    for batch in a.batch:
        runs = {leg: [] for leg in LEGS}
        for _ in range(a.rounds):
            for leg in LEGS:  # alternating, one process each
                env = dict(os.environ)
                env.pop("HERING_NO_BLINDROT_BATCH", None)
                if leg == "per_entry":
                    env["HERING_NO_BLINDROT_BATCH"] = "1"
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--batch", str(batch), "--seconds", str(a.seconds),
                                    "--n-lwe", str(a.n_lwe)], env=env, capture_output=True, text=True, timeout=900)
                if r.returncode != 0:
                    print(r.stdout + r.stderr, file=sys.stderr)
                    return 2
                line = r.stdout.strip().splitlines()[-1]
                print(line, flush=True)
                runs[leg].append(json.loads(line))
        med = {leg: float(np.median([x["ms"] for x in runs[leg]])) for leg in LEGS}
        same = len({x["digest"] for leg in LEGS for x in runs[leg]}) == 1
        bad += not same
        print(json.dumps(dict(batch=batch, n_lwe=a.n_lwe, median_ms=med, rotations_per_s={leg: batch / (med[leg] * 1e-3) for leg in LEGS},
                              spread_ms={leg: max(x["ms"] for x in runs[leg]) - min(x["ms"] for x in runs[leg]) for leg in LEGS},
                              launches={leg: runs[leg][0]["launches"] for leg in LEGS}, rounds=runs["batched"][0]["rounds"],
                              same_words=same, speedup_batched=med["per_entry"] / med["batched"])), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
