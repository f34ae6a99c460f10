#!/usr/bin/env python3
"""Times the RGSW external product (include/hering_rgsw.h) at the blind-rotation shapes, three ways:

  composed   the sequence a caller composes from the entry points the library had before: two he_gadget_product_lazy, the adds
             of their accumulators (Q, and P where there is one) and he_moddown -- the copy where there is no special prime.
             It calls none of the new entry points.
  generic    he_rgsw_external_product with HERING_NO_RGSW_FUSED=1
  fused      he_rgsw_external_product as dispatched (the one-launch kernel inside its domain)

    python tools/rgsw_bench.py [--shape lmkcdey b2] [--batch 1 256 4096] [--seconds 0.5]

  lmkcdey   logN 10, q = 0x7fff801, BaseTwoDecomposition 7, no special prime
  b2        logN 10, Q (35, 20 bits) + P (61 bits), BaseTwoDecomposition 7

Every configuration (shape, batch, leg) runs in a process of its own, so that the environment switch and the warm-up of one
leg cannot touch another: the parent starts a child per configuration, legs alternating, three rounds, and reports the median.
A child warms its shape up, sizes its repetition count to fill `--seconds`, times that many calls between device events, and
counts the launches of one call with the kernel profiler in a separate, untimed pass.  The results of the three legs are
compared word for word (a digest of the outputs on the same seeded inputs).  Exit status: non-zero when a digest differs, when
the fused leg is not faster than the composed one at some batch, or when the generic leg is slower than the composed one by
more than the spread of the composed leg's own rounds.  Prints one JSON line per (shape, batch) and one per child."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    "lmkcdey": dict(logN=10, q=[0x7FFF801], logp=[], pw2=7),
    "b2": dict(logN=10, logq=[35, 20], logp=[61], pw2=7),
}
LEGS = ("composed", "generic", "fused")


def child(shape, batch, leg, seconds):
    import lattigo_amd as la
    from lattigo_amd import _lib
    from oracle import oracle as O  # (prime generation only)

    sh = SHAPES[shape]
    N = 1 << sh["logN"]
    if "q" in sh:
        q, p = list(sh["q"]), []
    else:
        q, p = O.GenModuli(sh["logN"] + 1, sh["logq"], sh["logp"])
        q, p = list(q), list(p)
    pw2 = sh["pw2"]
    rng = np.random.default_rng(20261018)
    ctx = la.Context(0)
    gQ = la.Ring(ctx, N, q)
    gP = la.Ring(ctx, N, p) if p else None
    gev = la.Evaluator(gQ, gP)
    nj = [(int(x).bit_length() + pw2 - 1) // pw2 for x in q]
    D, L, LP = sum(nj), len(q), len(p)
    level = L - 1

    def polys(mod, n):
        return np.stack([np.stack([rng.integers(0, m, size=N, dtype=np.uint64) for m in mod]) for _ in range(n)])

    keys = []
    for _ in range(2):
        kq = polys(q, 2 * D).reshape(D, 2, L, N)
        kp = polys(p, 2 * D).reshape(D, 2, LP, N) if p else None
        keys.append(gev.NewEvaluationKey(kq, kp, pw2, nj))
    ct = [la.Poly(gQ, L, batch).upload(polys(q, batch)) for _ in range(2)]
    out = [la.Poly(gQ, L, batch) for _ in range(2)]
    Lib = _lib.load()

    if leg == "composed":
        accs = [[(la.Poly(gQ, L, batch), la.Poly(gP, LP, batch) if p else None) for _ in range(2)] for _ in range(2)]
        rQ, rP = gQ.AtLevel(level), (gP.AtLevel(LP - 1) if p else None)

        def call():
            for k in range(2):
                gev.GadgetProductLazy(level, ct[k], keys[k], accs[k])
            for c in range(2):
                rQ.binop("Add", accs[0][c][0], accs[1][c][0], accs[0][c][0])
                if p:
                    rP.binop("Add", accs[0][c][1], accs[1][c][1], accs[0][c][1])
            gev.ModDown(level, LP - 1, accs[0], out)
    else:
        def call():
            _lib.check(Lib.he_rgsw_external_product(gev.h, ct[0].h, ct[1].h, keys[0].h, keys[1].h, out[0].h, out[1].h))

    call()
    ctx.sync()
    digest = hashlib.sha256(b"".join(o.download().tobytes() for o in out)).hexdigest()[:16]
    ctx.prof_begin()
    call()
    prof = ctx.prof_end()
    launches = int(sum(n for n, _ in prof.values()))
    # steady state: warm up, size the window, then time it between device events
    for _ in range(3):
        call()
    ctx.sync()
    ctx.timer_start()
    for _ in range(5):
        call()
    per = max(ctx.timer_stop() / 5, 1e-3)  # ms
    reps = int(min(max(seconds * 1e3 / per, 10), 20000))
    ctx.timer_start()
    for _ in range(reps):
        call()
    ms = ctx.timer_stop() / reps
    print(json.dumps(dict(shape=shape, batch=batch, leg=leg, ms=ms, reps=reps, launches=launches, kernels={k: v[0] for k, v in prof.items()},
                          digest=digest)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--batch", nargs="+", type=int, default=[1, 256, 4096])
    ap.add_argument("--leg", choices=LEGS, help="run one configuration in this process (what the parent starts)")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.leg:
        child(a.shape[0], a.batch[0], a.leg, a.seconds)
        return 0
    bad = 0
    for shape in a.shape:
        for batch in a.batch:
            runs = {leg: [] for leg in LEGS}
            for _ in range(a.rounds):
                for leg in LEGS:  # alternating, one process each
                    env = dict(os.environ)
                    env.pop("HERING_NO_RGSW_FUSED", None)
                    if leg == "generic":
                        env["HERING_NO_RGSW_FUSED"] = "1"
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--shape", shape, "--batch", str(batch),
                                        "--seconds", str(a.seconds)], env=env, capture_output=True, text=True, timeout=600)
                    if r.returncode != 0:
                        print(r.stdout + r.stderr, file=sys.stderr)
                        return 2
                    line = r.stdout.strip().splitlines()[-1]
                    print(line, flush=True)
                    runs[leg].append(json.loads(line))
            med = {leg: float(np.median([x["ms"] for x in runs[leg]])) for leg in LEGS}
            spread = max(x["ms"] for x in runs["composed"]) - min(x["ms"] for x in runs["composed"])
            same = len({x["digest"] for leg in LEGS for x in runs[leg]}) == 1
            ok_fused = med["fused"] < med["composed"]
            ok_generic = med["generic"] <= med["composed"] + spread
            bad += (not same) + (not ok_fused) + (not ok_generic)
            print(json.dumps(dict(shape=shape, batch=batch, median_ms=med, composed_spread_ms=spread,
                                  launches={leg: runs[leg][0]["launches"] for leg in LEGS}, same_words=same,
                                  fused_over_composed=med["fused"] / med["composed"], generic_over_composed=med["generic"] / med["composed"],
                                  fused_faster=ok_fused, generic_not_slower=ok_generic)), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
