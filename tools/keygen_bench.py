#!/usr/bin/env python3
"""Times the generation of evaluation keys (lattigo_amd.keygen, include/hering_keygen.h) at logN 15, 12 + 3 moduli: one
relinearization key and a set of 24 Galois keys, from the system source and from a deterministic callback source, on two routes:

    fused      he_keygen_relinearization_key / he_keygen_galois_keys
    composed   the same rows from the public entries that existed before: Encryptor.EncryptZero on each row (a QP element under
               skOut), then he_gadget_add_poly on a key.  The rows stay in their polynomials: the copy into the key's storage that a
               real composition would also make is not counted, which favours this route.

    python tools/keygen_bench.py [--rounds 3] [--galois 24]

Per case: the wall-clock time of one generation (median over `--rounds` after a warm-up; a call returns with the device drained),
the device time of its launches by HIP events and their count from a separate profiled run (he_prof_end), the time the source
takes for the bytes consumed (os.getrandom, or the callback alone), and those bytes.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class CyclicSource:
    """a deterministic stream: a block of PCG64 bytes, served cyclically"""

    def __init__(self, seed=1, size=1 << 26):
        import numpy as np
        self.block = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size, dtype=np.uint8).tobytes()
        self.at = 0

    def read(self, n):
        out = bytearray()
        while n:
            take = min(n, len(self.block) - self.at)
            out += self.block[self.at:self.at + take]
            self.at = (self.at + take) % len(self.block)
            n -= take
        return bytes(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--galois", type=int, default=24)
    a = ap.parse_args()

    import lattigo_amd as la
    from lattigo_amd import encryptor as E
    from lattigo_amd import keygen as G
    from lattigo_amd import sampling
    from tests.rlwe_fixtures import downstream_primes

    logN, nq, npp = 15, 12, 3
    pr = downstream_primes(55, 2 << logN, nq + npp)
    ctx = la.Context(0)
    rq, rp = la.Ring(ctx, 1 << logN, pr[:nq]), la.Ring(ctx, 1 << logN, pr[nq:])
    ev = la.Evaluator(rq, rp)
    gal_els = [pow(5, k + 1, 2 << logN) for k in range(a.galois)]
    out = {"logN": logN, "limbs": [nq, npp], "rounds": a.rounds, "galois_keys": a.galois, "cases": []}
    for source in ("system", "callback"):
        cyc = CyclicSource() if source == "callback" else None
        prng = sampling.PRNG(cyc.read if cyc else None)
        kg = G.KeyGenerator(ev, prng)
        sk = kg.GenSecretKeyNew()
        rlk, gks = kg.NewEvaluationKey(), [kg.NewEvaluationKey() for _ in gal_els]
        rows = rlk.beta
        enc = E.Encryptor(ev, prng, sk)
        cts = [E.ElementQP([(rq.NewPoly(), rp.NewPoly()) for _ in range(2)], True, True) for _ in range(rows)]

        def composed(keys):
            for key in keys:
                for ct in cts:
                    enc.EncryptZero(ct)
                G.AddPolyTimesGadgetVectorToGadgetCiphertext(sk.Q, [key])

        calls = {("rlk", "fused"): lambda: kg.GenRelinearizationKey(sk, rlk), ("rlk", "composed"): lambda: composed([rlk]),
                 ("galois", "fused"): lambda: kg.GenGaloisKeys(gal_els, sk, gks), ("galois", "composed"): lambda: composed(gks)}
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
            out["cases"].append({"source": source, "keys": what, "route": route, "rows_per_key": rows, "wall_ms": round(statistics.median(walls), 3),
                                 "device_ms": round(sum(v[1] for v in prof.values()), 3), "launches": sum(v[0] for v in prof.values()),
                                 "kernels": {k: [v[0], round(v[1], 3)] for k, v in prof.items()}, "bytes_consumed": consumed,
                                 "source_ms": round(source_ms, 3)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
