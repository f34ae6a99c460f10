#!/usr/bin/env python3
"""Times Encrypt under pk, EncryptZero under sk and Decrypt (lattigo_amd.encryptor, include/hering_encryptor.h) on the system source
at the headline shape: logN 15, 12 + 3 moduli, batch 1 and 64.

    python tools/encryptor_bench.py [--rounds 5]

Per call and batch: the wall-clock time of one call (median over `--rounds` calls after a warm-up; a call returns with the device
drained), the device time of its launches and their count from a separate profiled call (he_prof_end), and the time os.getrandom
takes for the bytes the call consumes -- the floor that the host source sets.  wall - device is what the host spends fetching,
staging and wiping.  Prints one JSON line."""
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
    from lattigo_amd import encryptor as E
    from lattigo_amd import sampling
    from tests.rlwe_fixtures import downstream_primes

    logN, nq, npp = 15, 12, 3
    pr = downstream_primes(55, 2 << logN, nq + npp)
    ctx = la.Context(0)
    rq, rp = la.Ring(ctx, 1 << logN, pr[:nq]), la.Ring(ctx, 1 << logN, pr[nq:])
    ev = la.Evaluator(rq, rp)
    prng = sampling.PRNG()
    out = {"logN": logN, "limbs": [nq, npp], "rounds": a.rounds, "cases": []}
    for batch in (1, 64):
        # uniform words serve as keys: every launch does the same work on them
        uni = sampling.UniformSampler(prng, rq, rp)
        sk = E.SecretKey(*uni.ReadNew(batch))
        pk = E.PublicKey((uni.ReadNew(batch), uni.ReadNew(batch)))
        pt = E.Plaintext(sampling.UniformSampler(prng, rq).ReadNew(batch))
        ct = E.Element([rq.NewPoly(batch), rq.NewPoly(batch)])
        out_pt = E.Plaintext(rq.NewPoly(batch))
        enc_sk, enc_pk, dec = E.Encryptor(ev, prng, sk), E.Encryptor(ev, prng, pk), E.Decryptor(ev, sk)
        calls = {"encrypt_pk": lambda: enc_pk.Encrypt(pt, ct), "encrypt_zero_sk": lambda: enc_sk.EncryptZero(ct), "decrypt": lambda: dec.Decrypt(ct, out_pt)}
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
            out["cases"].append({"call": name, "batch": batch, "wall_ms": round(statistics.median(walls), 3),
                                 "device_ms": round(sum(v[1] for v in prof.values()), 3), "launches": sum(v[0] for v in prof.values()),
                                 "kernels": {k: [v[0], round(v[1], 3)] for k, v in prof.items()}, "bytes_consumed": consumed,
                                 "getrandom_ms": round(source_ms, 3)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
