#!/usr/bin/env python3
"""Times a party's key-sized shares of the multiparty protocols (lattigo_amd.multiparty, include/hering_multiparty.h) at logN 15,
12 + 3 moduli, from the system source, on two routes:

    fused      he_mp_evk_gen_share, he_mp_rkg_round_one, he_mp_rkg_round_two: the draws row by row, then two expansions, one
               transform and one launch over every row
    composed   the same share row by row from the entries that existed before: the Gaussian Read, the extension to P, NTT, MForm and
               the products per row, on polynomials.  This is the baseline, not the code under test.  The rows stay in their
               polynomials (the copy into a key's storage is not counted) and the gadget term of round one is left out, both of which
               favour this route.

    python tools/multiparty_bench.py [--rounds 5]

Per case: the wall-clock time of one share (median over `--rounds` after a warm-up; a call returns with the device drained), the
device time of its launches by HIP events and their count from a separate profiled run (he_prof_end), and the bytes consumed.
Prints one JSON line."""
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
    from lattigo_amd import keygen as G
    from lattigo_amd import multiparty as MP
    from lattigo_amd import sampling
    from lattigo_amd._lib import check, load
    from tests.rlwe_fixtures import downstream_primes

    L = load()
    logN, nq, npp = 15, 12, 3
    pr = downstream_primes(55, 2 << logN, nq + npp)
    ctx = la.Context(0)
    rq, rp = la.Ring(ctx, 1 << logN, pr[:nq]), la.Ring(ctx, 1 << logN, pr[nq:])
    ev = la.Evaluator(rq, rp)
    prng = sampling.PRNG(None)
    kg = G.KeyGenerator(ev, prng)
    sk, sk2 = kg.GenSecretKeyNew(), kg.GenSecretKeyNew()
    evk, rkg = MP.EvaluationKeyGenProtocol(kg), MP.RelinearizationKeyGenProtocol(kg)
    crp = evk.SampleCRP(sampling.PRNG(None))
    share = evk.AllocateShare()
    eph, r1, r2 = rkg.AllocateShare()
    rows = share.key.beta
    lq, lp = nq - 1, npp - 1
    SUB, LAZY, THEN_ADD, THEN_SUB = 2, 9, 11, 14  # he_binop codes (include/hering.h)
    new = lambda: (rq.NewPoly(), rp.NewPoly())
    crp_rows = [sampling.UniformSampler(prng, rq, rp).ReadNew() for _ in range(rows)]  # the CRP as polynomials, row by row
    h_rows = [(new(), new()) for _ in range(rows)]
    out_rows = [(new(), new()) for _ in range(rows)]
    e = new()
    d = new()

    def gauss(dst):  # sampler.Read; ExtendBasisSmallNormAndCenter; NTT
        check(L.he_sampler_gaussian_read(rq.h, lq, prng.h, 3.2, 19.2, 0, 0, dst[0].h))
        check(L.he_centered_lift(ev.h, 3, dst[0].h, lq + 1, lq, dst[0].h, lp, dst[1].h))
        check(L.he_ntt(rq.h, lq, dst[0].h, dst[0].h))
        check(L.he_ntt(rp.h, lp, dst[1].h, dst[1].h))

    def both(op, x, y, z):
        check(L.he_binop(rq.h, lq, op, x[0].h, y[0].h, z[0].h))
        check(L.he_binop(rp.h, lp, op, x[1].h, y[1].h, z[1].h))

    def composed_evk():
        for r in range(rows):
            o = out_rows[r][0]
            gauss(o)
            check(L.he_mform(rq.h, lq, o[0].h, o[0].h))
            check(L.he_mform(rp.h, lp, o[1].h, o[1].h))
            both(THEN_SUB, crp_rows[r], (sk2.Q, sk2.P), o)
        G.AddPolyTimesGadgetVectorToGadgetCiphertext(sk.Q, [share.key])

    def composed_round_one():
        for r in range(rows):
            o0, o1 = out_rows[r]
            gauss(o0)
            both(THEN_SUB, (eph.Q, eph.P), crp_rows[r], o0)
            gauss(o1)
            both(THEN_ADD, (sk.Q, sk.P), crp_rows[r], o1)

    def composed_round_two():
        both(SUB, (eph.Q, eph.P), (sk.Q, sk.P), d)
        for r in range(rows):
            o = out_rows[r][0]
            both(LAZY, h_rows[r][0], (sk.Q, sk.P), o)
            gauss(e)
            both(0, o, e, o)  # Add
            both(THEN_ADD, d, h_rows[r][1], o)

    calls = {("evk_gen_share", "fused"): lambda: evk.GenShare(sk, sk2, crp, share), ("evk_gen_share", "composed"): composed_evk,
             ("rkg_round_one", "fused"): lambda: rkg.GenShareRoundOne(sk, crp, eph, r1), ("rkg_round_one", "composed"): composed_round_one,
             ("rkg_round_two", "fused"): lambda: rkg.GenShareRoundTwo(eph, sk, r1, r2), ("rkg_round_two", "composed"): composed_round_two}
    out = {"logN": logN, "limbs": [nq, npp], "rows": rows, "rounds": a.rounds, "cases": []}
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
        out["cases"].append({"share": what, "route": route, "wall_ms": round(statistics.median(walls), 3), "wall_ms_all": [round(w, 3) for w in walls],
                             "device_ms": round(sum(v[1] for v in prof.values()), 3), "launches": sum(v[0] for v in prof.values()),
                             "kernels": {k: [v[0], round(v[1], 3)] for k, v in prof.items() if v[0]}, "bytes_consumed": consumed})
    for what in ("evk_gen_share", "rkg_round_one", "rkg_round_two"):
        f, c = [next(x for x in out["cases"] if x["share"] == what and x["route"] == r) for r in ("fused", "composed")]
        out[what + "_composed_over_fused_wall"] = round(c["wall_ms"] / f["wall_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
