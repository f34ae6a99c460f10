#!/usr/bin/env python3
"""Times the one-launch forms of include/hering_ckks_evaluator.h against the composed sequences of the ring-level entries a caller
had before them, in the same process, on the same words:

    ct x pt Mul                     MForm into a temporary + a product per component          | he_ckks_mul_pt
    ct x pt MulThenAdd, scale-up    a scalar product per accumulator component + the above    | he_ckks_mul_pt(then_add, pre)
    Add of different scales         a scalar product per component into a temporary + Add     | he_ckks_add(scaled)
    ct x ct MulThenAdd              two MForm + four MulCoeffsMontgomeryThenAdd               | he_ckks_mul_relin_then_add (no key)
    MulRelinThenAdd                 the same with the c2 product + he_relinearize in place    | he_ckks_mul_relin_then_add (key)

    python tools/ckks_evaluator_bench.py [--shape c2 | c5] [--out profiles/ckks_evaluator_bench_c2.json]

Shapes: c2 = logN 14, 8 + 2 moduli, batch 256 (bench.py's); c5 = logN 16, 25 + 5 moduli, batch 32.  Words are synthetic uniform
residues (throughput does not depend on their values; tests/test_gpu_ckks_evaluator.py holds the words against the reference).
Per form: both legs are warmed up, a window of about 0.2 s is sized from three calls, and three windows per leg are timed
between device events (he_timer_*), the legs alternating; the figure is the median, the spread (max - min) / median of the three.
The fused kernel's bytes are the launcher's own accounting (he_prof_end_bytes), its fraction of HBM peak bytes / time / 8 TB/s.
Prints (and writes) one JSON document."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PEAK_HBM = 8.0e12
WINDOW_MS = 200.0
SHAPES = {"c2": (14, [55] + [45] * 7, [55] * 2, 256), "c5": (16, [60] + [40] * 9 + [39] * 3 + [60] * 8 + [56] * 4, [61] * 5, 32)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="c2", choices=sorted(SHAPES))
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import lattigo_amd as la
    from bench import uniform
    from bootstrap_c5_shape import gen_primes
    from lattigo_amd import ckks as K

    logN, logq, logp, B = SHAPES[a.shape]
    B = a.batch or B
    N, nth, taken = 1 << logN, 2 << logN, set()
    q, p = gen_primes(logq, nth, taken), gen_primes(logp, nth, taken)
    L, level = len(q), len(q) - 1
    ctx = la.Context(0)
    rq, rp = la.Ring(ctx, N, q), la.Ring(ctx, N, p)
    ev = la.Evaluator(rq, rp)
    rng = np.random.Generator(np.random.PCG64(0xC4E5 + logN))

    def poly():
        x = la.Poly(rq, L, B)
        row = uniform(rng, q, N)
        for b in range(B):  # (the same words in every entry: uploads of a full batch would dominate the set-up)
            for i in range(L):
                x.upload_limb(b, i, row[i])
        return x

    beta = -(-L // len(p))
    kq, kp = uniform(rng, q, N, (beta, 2)), uniform(rng, p, N, (beta, 2))
    rlk = ev.NewEvaluationKey(kq, kp)
    a0, a1, b0, b1, c0, c1, c2, t0, t1, t2, pt = (poly() for _ in range(11))
    words = np.array([int(rng.integers(1, m)) for m in q], dtype=np.uint64)

    def composed_mul_pt():
        rq.unop("MForm", pt, t0)
        rq.binop("MulCoeffsMontgomery", a0, t0, c0)
        rq.binop("MulCoeffsMontgomery", a1, t0, c1)

    def composed_mul_pt_then_add():
        rq.MulDoubleRNSScalar(c0, words, words, c0)
        rq.MulDoubleRNSScalar(c1, words, words, c1)
        rq.unop("MForm", pt, t0)
        rq.binop("MulCoeffsMontgomeryThenAdd", a0, t0, c0)
        rq.binop("MulCoeffsMontgomeryThenAdd", a1, t0, c1)

    def composed_add_scaled():
        rq.MulDoubleRNSScalar(b0, words, words, t0)
        rq.MulDoubleRNSScalar(b1, words, words, t1)
        rq.binop("Add", a0, t0, c0)
        rq.binop("Add", a1, t1, c1)

    def composed_tensor(relin):
        rq.unop("MForm", a0, t0)
        rq.unop("MForm", a1, t1)
        rq.binop("MulCoeffsMontgomeryThenAdd", t0, b0, c0)
        rq.binop("MulCoeffsMontgomeryThenAdd", t0, b1, c1)
        rq.binop("MulCoeffsMontgomeryThenAdd", t1, b0, c1)
        if relin:
            rq.binop("MulCoeffsMontgomery", t1, b1, t2)
            ev.Relinearize(level, [c0, c1, t2], rlk, [c0, c1])
        else:
            rq.binop("MulCoeffsMontgomeryThenAdd", t1, b1, c2)

    forms = {
        "mul_pt": (composed_mul_pt, lambda: K.ct_mul_pt(rq, [a0, a1], pt, [c0, c1]), "ct_lin", (8, 5)),
        "mul_pt_then_add_scaled": (composed_mul_pt_then_add, lambda: K.ct_mul_pt(rq, [a0, a1], pt, [c0, c1], then_add=True, pre=words), "ct_lin", (14, 7)),
        "add_scaled": (composed_add_scaled, lambda: K.ct_add(rq, [a0, a1], [b0, b1], [c0, c1], scaled=2, ratio=words), "ct_lin", (10, 6)),
        "mul_then_add_ct": (lambda: composed_tensor(False), lambda: K.ct_mul_relin_then_add(ev, level, [a0, a1], [b0, b1], None, [c0, c1, c2]),
                            "tensor_add", (20, 10)),
        "mul_relin_then_add": (lambda: composed_tensor(True), lambda: K.ct_mul_relin_then_add(ev, level, [a0, a1], [b0, b1], rlk, [c0, c1]),
                               "tensor_add", (25, 9)),
    }

    def window(fn, n):
        ctx.sync()
        ctx.timer_start()
        for _ in range(n):
            fn()
        return ctx.timer_stop() / n

    out = {"shape": a.shape, "logN": logN, "limbs": L, "batch": B, "forms": {}}
    for name, (composed, fused, kernel, passes) in forms.items():
        for fn in (composed, fused):
            for _ in range(3):
                fn()
        ctx.sync()
        n = max(3, int(WINDOW_MS / max(window(composed, 3), 1e-3)))
        tc, tf = [], []
        for _ in range(3):
            tc.append(window(composed, n))
            tf.append(window(fused, n))
        ctx.prof_begin()
        fused()
        ctx.sync()
        prof = ctx.prof_end_bytes()
        _, kms, kbytes = prof[kernel]
        mc, mf = float(np.median(tc)), float(np.median(tf))
        out["forms"][name] = {
            "composed_ms": mc, "fused_ms": mf, "ratio_composed_over_fused": mc / mf,
            "spread_composed": (max(tc) - min(tc)) / mc, "spread_fused": (max(tf) - min(tf)) / mf,
            "passes_expected": {"composed": passes[0], "fused": passes[1]},
            "kernel": kernel, "kernel_ms": kms, "kernel_bytes": kbytes, "kernel_hbm_fraction": kbytes / (kms * 1e-3) / PEAK_HBM,
            "launches": {k: v[0] for k, v in prof.items()}, "calls_per_window": n}
    doc = json.dumps(out)
    print(doc)
    if a.out:
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
