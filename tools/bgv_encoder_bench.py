#!/usr/bin/env python3
"""Times the device encoder of BGV / BFV (lattigo_amd.bgv.Encoder, include/hering_bgv_encoder.h) against the only way the tree
could encode and decode before it: the restatement of the reference on the CPU (tests/bgv_encoder_ref.py, the oracle's C
transforms with Python integers between them) plus the upload / download of the words.

    python tools/bgv_encoder_bench.py [--vectors 256] [--plaintexts 64] [--host-vectors 2] [--rounds 3]

Two parameter sets, T = 65537, 12 + 3 moduli: logN 15 (N_T = N, gap 1) and logN 16 (N_T = 2^15, gap 2: the case real parameters
hit).  Per set: EncodeQP of `vectors` full slot vectors (NTT + Montgomery form) as ONE batched call; Decode of `plaintexts`
NTT-domain plaintexts as one batched call at the top level and at level 0.  The host leg runs `host-vectors` of them, one at a
time, and its figure is per vector.  Times are host wall-clock around calls that end with the device drained, after a warm-up of
each leg; a device leg repeats its call until the timed window is about 0.3 s; the figure is the median over `--rounds` rounds.
Launch counts come from a separate profiled call (he_prof_end) and must equal the census: 2 new launches plus what the existing
transforms launch for ringT and ringQ (and ringP) at these sizes, whatever the batch -- the tool exits 1 otherwise, or when the
two legs disagree on a word.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW_MS = 300.0
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=256)
    ap.add_argument("--plaintexts", type=int, default=64)
    ap.add_argument("--host-vectors", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()

    import lattigo_amd as la
    from lattigo_amd import bgv
    from oracle import oracle as O
    from tests import bgv_encoder_ref as R

    ctx = la.Context(0)
    T = 65537
    med = lambda v: float(np.median(v))

    def census(call):
        ctx.sync()
        ctx.prof_begin()
        call()
        ctx.sync()
        return {k: v[0] for k, v in ctx.prof_end().items()}

    def wall(call, window_ms=0.0):
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

    ok, res = True, {}
    for logN in (15, 16):
        N = 1 << logN
        q, p = O.GenModuli(logN + 1, [55] * 12, [55] * 3)
        q, p = [int(x) for x in q], [int(x) for x in p]
        P = R.Params(logN, q, T, p)
        gQ, gP, gT = la.Ring(ctx, N, q), la.Ring(ctx, N, p), la.Ring(ctx, P.NT, [T])
        enc = bgv.Encoder(gQ, gT, gP)
        rng = np.random.default_rng(logN)
        D, B, H, top = a.vectors, a.plaintexts, a.host_vectors, len(q) - 1
        v = rng.integers(0, T, (D, P.NT), dtype=np.uint64)
        scale = 3

        # ---- EncodeQP
        pq, pp = la.Poly(gQ, len(q), D, zero=False), la.Poly(gP, len(p), D, zero=False)
        hq, hp = la.Poly(gQ, len(q), 1, zero=False), la.Poly(gP, len(p), 1, zero=False)
        native_enc = lambda: enc.EncodeQP(v, pq, pp, Scale=scale)

        def host_enc():
            out = []
            for i in range(H):
                pT = P.encode_ring_t(v[i], scale, False)
                wq = P._finish(P.ring_t2q(pT, top, False), False, top, True, True)
                wp = P._finish(P.ring_t2q(pT, len(p) - 1, False, True), True, len(p) - 1, True, True)
                hq.upload(wq)
                hp.upload(wp)
                out.append((wq, wp))
            return out

        native_enc()
        want = host_enc()
        got_q, got_p = pq.download(), pp.download()
        ok &= all(np.array_equal(got_q[i], want[i][0]) and np.array_equal(got_p[i], want[i][1]) for i in range(H))
        ms_enc = {"native": [wall(native_enc, WINDOW_MS) for _ in range(a.rounds)], "host": [wall(host_enc) for _ in range(a.rounds)]}
        one_q, one_p, one_t = la.Poly(gQ, len(q)), la.Poly(gP, len(p)), la.Poly(gT, 1)
        parts = [census(lambda: gT.INTT(one_t, one_t)), census(lambda: gQ.NTT(one_q, one_q)), census(lambda: gP.NTT(one_p, one_p))]
        expect_enc = 2 + sum(sum(c.values()) for c in parts)
        launches_enc = census(native_enc)
        ok &= sum(launches_enc.values()) == expect_enc and launches_enc.get("bgv_slots_to_t") == 1 and launches_enc.get("bgv_t_to_rns") == 1

        # ---- Decode at the top level and at level 0
        dec = {}
        for level in (top, 0):
            rq = gQ.AtLevel(level)
            pt = la.Poly(gQ, level + 1, B, zero=False)
            enc.Encode(v[:B], pt, Scale=scale, level=level)
            words = pt.download()
            singles = [la.Poly(gQ, level + 1, 1).upload(words[i]) for i in range(H)]
            native_dec = lambda: enc.Decode(pt, Scale=scale, level=level)
            host_dec = lambda: [P.decode(s.get(), scale, level, True, True, False) for s in singles]
            got, hw = native_dec(), host_dec()
            ok &= np.array_equal(got, v[:B]) and all(np.array_equal(hw[i], v[i]) for i in range(H))
            ms = {"native": [wall(native_dec, WINDOW_MS) for _ in range(a.rounds)], "host": [wall(host_dec) for _ in range(a.rounds)]}
            one = la.Poly(gQ, level + 1)
            expect = 2 + sum(census(lambda: rq.INTT(one, one)).values()) + sum(census(lambda: gT.NTT(one_t, one_t)).values())
            launches = census(native_dec)
            ok &= sum(launches.values()) == expect and launches.get("bgv_rns_to_t") == 1 and launches.get("bgv_t_to_slots") == 1
            dec[f"level{level}"] = dict(plaintexts=B, native_ms=med(ms["native"]), native_ms_per_plaintext=med(ms["native"]) / B,
                                        host_ms_per_plaintext=med(ms["host"]) / H, host_over_native=(med(ms["host"]) / H) / (med(ms["native"]) / B),
                                        launches=launches, census=expect, rounds=ms)
        res[f"logN{logN}"] = dict(
            moduli=f"{len(q)}+{len(p)}", T=T, logNT=P.logNT, gap=P.gap,
            encode_qp=dict(vectors=D, host_vectors=H, native_ms=med(ms_enc["native"]), native_ms_per_vector=med(ms_enc["native"]) / D,
                           host_ms_per_vector=med(ms_enc["host"]) / H, host_over_native=(med(ms_enc["host"]) / H) / (med(ms_enc["native"]) / D),
                           launches=launches_enc, census=expect_enc, rounds=ms_enc),
            decode=dec)
    res["ok"] = bool(ok)
    print(json.dumps(res), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
