#!/usr/bin/env python3
"""Times the device encoder (lattigo_amd.ckks.Encoder, include/hering_ckks_encoder.h) against tests/drivers/dft.py::Encoder, the
only encoder the tree had before it: numpy special (i)FFT and rounding on the host, a Python big-integer CRT per coefficient for
decode.

    python tools/ckks_encoder_bench.py [--logN 16] [--diagonals 256] [--plaintexts 64] [--driver-plaintexts 4]

Encode: EncodeQP of `diagonals` full slot vectors at logN, 25 + 5 moduli, NTT + Montgomery form (what encoding the CoeffsToSlots /
SlotsToCoeffs matrices of a bootstrapping set-up costs) -- the product as ONE batched call, the driver one vector at a time.
Decode: `plaintexts` NTT-domain plaintexts at level 9 -- the product as one batched call; the driver decodes `driver-plaintexts`
of them (each is N big-integer reconstructions in Python) and its figure is per plaintext.
Times are host wall-clock around calls that end with the device drained (both encoders move host data, so the host's share is
what is being measured), after a warm-up of each leg at the timed shape; a product leg repeats its call until the timed window is
about 0.3 s and reports the time per call; the legs alternate over `--rounds` rounds and the figure is the median.
Small: the one-workgroup route (iFFT and quantiser in ONE launch per call) at logN 14, 2^13 slots, 25 + 5 moduli, batch 1, 16 and
64 -- the product alone (per call and per vector), since one workgroup per vector writes all its limbs.  Launch counts come from a separate profiled call (he_prof_end).  The two encoders do not produce the same words
(the driver rounds half-to-even and casts through int64): the check here is that both decode each other's plaintexts back to the
input within the CKKS bound.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW_MS = 300.0  # a timed window of a product leg
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logN", type=int, default=16)
    ap.add_argument("--diagonals", type=int, default=256)
    ap.add_argument("--plaintexts", type=int, default=64)
    ap.add_argument("--driver-plaintexts", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()

    import lattigo_amd as la
    from drivers import dft as DRV
    from lattigo_amd import ckks
    from oracle import oracle as O

    logN, N, n = a.logN, 1 << a.logN, 1 << (a.logN - 1)
    q, p = O.GenModuli(logN + 1, [55] + [45] * 24, [55] * 5)
    q, p = [int(x) for x in q], [int(x) for x in p]
    ctx = la.Context(0)
    gQ, gP = la.Ring(ctx, N, q), la.Ring(ctx, N, p)
    enc, drv = ckks.Encoder(gQ, gP), DRV.Encoder(gQ, gP)
    rng = np.random.default_rng(logN)
    D, B, level, scale = a.diagonals, a.plaintexts, 9, 2.0 ** 45
    z = rng.uniform(-1, 1, (D, n)) + 1j * rng.uniform(-1, 1, (D, n))

    def census(call):
        ctx.sync()
        ctx.prof_begin()
        call()
        ctx.sync()
        return {k: v[0] for k, v in ctx.prof_end().items()}

    def wall(call, window_ms=0.0):
        """ms per call; window_ms: repeat the call until the window is about that long"""
        ctx.sync()
        t = time.perf_counter()
        call()
        ctx.sync()
        one = (time.perf_counter() - t) * 1e3
        reps = int(min(max(window_ms / max(one, 1e-3), 1), 1000))
        if reps == 1:
            return one
        t = time.perf_counter()
        for _ in range(reps):
            call()
        ctx.sync()
        return (time.perf_counter() - t) * 1e3 / reps

    # ---- encode
    pq, pp = la.Poly(gQ, len(q), D, zero=False), la.Poly(gP, len(p), D, zero=False)
    native_enc = lambda: enc.EncodeQP(z, pq, pp, Scale=scale)
    driver_enc = lambda: [drv.EncodeQP(z[i], len(q) - 1, scale) for i in range(D)]
    native_enc()
    driver_enc()
    ms_enc = {"native": [], "driver": []}
    for _ in range(a.rounds):
        ms_enc["native"].append(wall(native_enc, WINDOW_MS))
        ms_enc["driver"].append(wall(driver_enc))
    launches_enc = {"native": census(native_enc), "driver_per_diagonal": census(lambda: drv.EncodeQP(z[0], len(q) - 1, scale))}

    # ---- decode at level 9
    pt = la.Poly(gQ, level + 1, B, zero=False)
    enc.Encode(z[:B], pt, Scale=scale, level=level)
    dn = min(a.driver_plaintexts, B)
    singles = []
    for i in range(dn):
        s = la.Poly(gQ, level + 1, 1, zero=False)
        s.CopyBatch(level, 0, pt, i, 1)
        singles.append(s)
    native_dec = lambda: enc.Decode(pt, Scale=scale, level=level)
    driver_dec = lambda: [drv.Decode(s, scale) for s in singles]
    got_native = native_dec()
    got_driver = driver_dec()
    bound = 2.0 ** -(45 - (logN + 2))
    err_native = float(np.max(np.abs(got_native - z[:B])))
    err_driver = float(max(np.max(np.abs(got_driver[i] - z[i])) for i in range(dn)))
    # each decodes the other's encoding
    dq, _ = drv.EncodeQP(z[0], level, scale)
    imf = gQ.AtLevel(level)
    imf.IMForm(dq, dq)
    err_cross = float(np.max(np.abs(enc.Decode(dq, Scale=scale, level=level)[0] - z[0])))
    ms_dec = {"native": [], "driver": []}
    for _ in range(a.rounds):
        ms_dec["native"].append(wall(native_dec, WINDOW_MS))
        ms_dec["driver"].append(wall(driver_dec))
    launches_dec = {"native": census(native_dec), "driver_per_plaintext": census(lambda: drv.Decode(singles[0], scale))}

    med = lambda v: float(np.median(v))
    # ---- the one-workgroup route at small batch
    sN, sn = 1 << 14, 1 << 13
    sq, sp = O.GenModuli(15, [55] + [45] * 24, [55] * 5)
    sq, sp = [int(x) for x in sq], [int(x) for x in sp]
    hQ, hP = la.Ring(ctx, sN, sq), la.Ring(ctx, sN, sp)
    senc = ckks.Encoder(hQ, hP)
    small = {}
    for b in (1, 16, 64):
        zs = z[:b, :sn].copy()
        oq, op = la.Poly(hQ, len(sq), b, zero=False), la.Poly(hP, len(sp), b, zero=False)
        call = lambda: senc.EncodeQP(zs, oq, op, Scale=scale)
        call()
        ms = med([wall(call, WINDOW_MS) for _ in range(a.rounds)])
        small[b] = dict(ms_per_call=ms, ms_per_vector=ms / b, launches=census(call))
    res = dict(
        logN=logN, moduli=f"{len(q)}+{len(p)}",
        encode=dict(diagonals=D, native_ms=med(ms_enc["native"]), driver_ms=med(ms_enc["driver"]), rounds=ms_enc,
                    native_ms_per_diagonal=med(ms_enc["native"]) / D, driver_ms_per_diagonal=med(ms_enc["driver"]) / D,
                    driver_over_native=med(ms_enc["driver"]) / med(ms_enc["native"]), launches=launches_enc,
                    native_launches=sum(launches_enc["native"].values()), driver_launches=D * sum(launches_enc["driver_per_diagonal"].values())),
        decode=dict(level=level, plaintexts=B, driver_plaintexts=dn, native_ms=med(ms_dec["native"]), driver_ms=med(ms_dec["driver"]), rounds=ms_dec,
                    native_ms_per_plaintext=med(ms_dec["native"]) / B, driver_ms_per_plaintext=med(ms_dec["driver"]) / dn,
                    driver_over_native_per_plaintext=(med(ms_dec["driver"]) / dn) / (med(ms_dec["native"]) / B), launches=launches_dec),
        small=dict(logN=14, slots=sn, moduli=f"{len(sq)}+{len(sp)}", batches=small),
        errors=dict(bound=bound, native_round_trip=err_native, driver_round_trip=err_driver, native_decodes_driver_encoding=err_cross))
    print(json.dumps(res), flush=True)
    return 0 if max(err_native, err_driver, err_cross) <= bound else 1


if __name__ == "__main__":
    sys.exit(main())
