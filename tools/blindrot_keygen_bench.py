#!/usr/bin/env python3
"""Times the generation of the RGSW ciphertexts of a blind-rotation key set (lattigo_amd.rgsw.Encryptor, include/hering_rgsw_encryptor.h)
at logN 10, Q = [0x7FFF801], no special prime, BaseTwoDecomposition 7 (4 rows per gadget ciphertext), 512 LWE coefficients, from the
system source and from a deterministic callback source, on two routes:

    fused      he_rgsw_encrypt_table over the 512 ciphertexts (the table entry blindrot.GenEvaluationKeyNew runs)
    composed   the same rows from the public entries that existed before: Encryptor.EncryptZero on each row of Value[0] and Value[1]
               in turn, then he_gadget_add_poly with two keys per ciphertext.  The rows stay in their polynomials: the copy into
               the keys' storage that a real composition would also make is not counted, which favours this route.

and, on the fused route only, blindrot.GenEvaluationKeyNew as a whole (the key allocations and the 11 Galois keys included).

    python tools/blindrot_keygen_bench.py [--rounds 3] [--lwe 512] [--logn 10]

Per case: the wall-clock time of one generation (median over `--rounds` after a warm-up; a call returns with the device drained),
the device time of its launches by HIP events and their count from a separate profiled run (he_prof_end), of which the launches
after the draws (everything but the sampler parses), the time the source takes for the bytes consumed (os.getrandom, or the
callback alone), and those bytes.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.keygen_bench import CyclicSource  # noqa: E402

Q27 = 0x7FFF801
DRAWS = ("sampler_uniform", "sampler_uniform_chain", "sampler_gaussian")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lwe", type=int, default=512)
    ap.add_argument("--logn", type=int, default=10)
    a = ap.parse_args()

    import numpy as np

    import lattigo_amd as la
    from lattigo_amd import blindrot as B
    from lattigo_amd import encryptor as E
    from lattigo_amd import keygen as G
    from lattigo_amd import rgsw, sampling

    N, pw2, q_lwe = 1 << a.logn, 7, 0x3001
    ctx = la.Context(0)
    rq = la.Ring(ctx, N, [Q27])
    ev = rgsw.Evaluator(rq, None)
    rl = la.Ring(ctx, a.lwe, [q_lwe])
    params = G.EvaluationKeyParameters(0, -1, pw2)
    # the monomials X^0, X^1, X^-1 (NTT, Montgomery) and a ternary LWE secret's selection among them
    mono = np.zeros((3, 1, N), dtype=np.uint64)
    mono[0, 0, 0], mono[1, 0, 1], mono[2, 0, N - 1] = 1, 1, Q27 - 1
    pts = la.Poly(rq, 1, 3).upload(mono)
    rq.NTT(pts, pts)
    rq.MForm(pts, pts)
    one = [la.Poly(rq, 1, 1) for _ in range(3)]
    for s in range(3):
        one[s].CopyBatch(0, 0, pts, s, 1)
    sel = np.random.default_rng(7).integers(0, 3, a.lwe).astype(np.int32)
    out = {"logN": a.logn, "Q": [Q27], "pw2": pw2, "lwe": a.lwe, "rounds": a.rounds, "cases": []}
    for source in ("system", "callback"):
        cyc = CyclicSource() if source == "callback" else None
        prng = sampling.PRNG(cyc.read if cyc else None)
        kg = G.KeyGenerator(ev, prng)
        sk = kg.GenSecretKeyNew()
        skl = G.KeyGenerator(la.Evaluator(rl, None), prng).GenSecretKeyNew()
        cts = [rgsw.NewCiphertext(ev, 0, -1, pw2) for _ in range(a.lwe)]
        rows = cts[0].Value[0].beta
        genc = rgsw.Encryptor(ev, prng, sk)
        enc = E.Encryptor(ev, prng, sk)
        row_cts = [E.ElementQP([(rq.NewPoly(), None) for _ in range(2)], True, True, 0, -1) for _ in range(2 * rows)]

        def composed():
            for k, ct in enumerate(cts):
                for row in row_cts:
                    enc.EncryptZero(row)
                G.AddPolyTimesGadgetVectorToGadgetCiphertext(one[sel[k]], ct.Value)

        calls = {("rgsw", "fused"): lambda: genc.EncryptTable(pts, sel, cts), ("rgsw", "composed"): composed,
                 ("GenEvaluationKeyNew", "fused"): lambda: B.GenEvaluationKeyNew(ev, sk, rl, skl, params, prng=prng)}
        for (what, route), call in calls.items():
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
                left -= len(cyc.read(min(left, 1 << 24)) if cyc else os.getrandom(min(left, 1 << 24)))
            source_ms = (time.perf_counter() - t0) * 1e3
            out["cases"].append({"source": source, "keys": what, "route": route, "rows_per_gadget_ciphertext": rows,
                                 "wall_ms": round(statistics.median(walls), 3), "device_ms": round(sum(v[1] for v in prof.values()), 3),
                                 "device_ms_after_the_draws": round(sum(v[1] for k, v in prof.items() if k not in DRAWS), 3),
                                 "launches": sum(v[0] for v in prof.values()), "kernels": {k: [v[0], round(v[1], 3)] for k, v in prof.items()},
                                 "bytes_consumed": consumed, "source_ms": round(source_ms, 3)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
