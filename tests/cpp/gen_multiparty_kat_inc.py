#!/usr/bin/env python3
"""Known-answer words of tests/cpp/multiparty_mirror.cpp from the restatement of the reference (tests/multiparty_ref.py), as a C++
include: python gen_multiparty_kat_inc.py > multiparty_kat.inc.  Three streams -- the party's, the common reference string and the
smudging noise of the public-key switch -- each splitmix64 of (seed + k + block) per 8-byte block, which the program restates; the
answers are FNV-1a checksums over the words of each object and the positions of the party's source and of the second source the
call read (the CRS or the noise source; 0: none).  The same answers with exp / log moved 4 ulps up and down are asserted equal here,
so that none depends on the device's exp / log."""
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

import numpy as np  # noqa: E402

from oracle import oracle as O  # noqa: E402
from tests import keygen_ref as KR  # noqa: E402
from tests import multiparty_ref as MR  # noqa: E402
from tests import sampler_ref as R  # noqa: E402
from tests.conftest import Pi60, Qi60  # noqa: E402

LOGN, Q, P, SEED = 5, Qi60[:3], Pi60[:1], 0x9E3779B97F4A7C15
NOISE_SIGMA, NOISE_FRESH_SK = 25.6, 3.2
M64 = (1 << 64) - 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def source(k):
    def gen(off, n):
        out = bytearray()
        for o in range(off, off + n):
            out.append((splitmix64((SEED + (k << 32) + (o >> 3)) & M64) >> (8 * (o & 7))) & 0xFF)
        return bytes(out)
    return R.Source(gen)


def fnv(*words):
    h = 0xCBF29CE484222325
    for a in words:
        for w in np.asarray(a, dtype=np.uint64).ravel():
            h = ((h ^ int(w)) * 0x100000001B3) & M64
    return h


def answers(exp=math.exp, log=R._log):
    """[(name, checksum, position of the party's source, position of the other source)] in the order the program makes its calls"""
    N, lq, lp = 1 << LOGN, len(Q) - 1, len(P) - 1
    oQ, oP = O.Ring(N, Q), O.Ring(N, P)
    src, crs, noise = source(0), source(1), source(2)
    kw = dict(exp=exp, log=log)
    kg = KR.KeyGenerator(oQ, oP, src, **kw)
    out = []
    sk = kg.gen_secret_key(lq, lp)
    out.append(("sk", fnv(sk[0], sk[1]), src.pos, 0))
    pkp = MR.PublicKeyGenProtocol(oQ, oP, src, **kw)
    pcrp = pkp.sample_crp(crs)
    out.append(("pk_crp", fnv(pcrp[0], pcrp[1]), src.pos, crs.pos))
    share = pkp.gen_share(sk, pcrp)
    out.append(("pk_share", fnv(share[0], share[1]), src.pos, 0))
    crp = MR.sample_crp(oQ, oP, crs, lq, lp)
    zero = {"q": np.zeros_like(crp["q"]), "p": np.zeros_like(crp["p"])}
    key = lambda c0, c1: KR.image(MR.EvaluationKeyGenProtocol(oQ, oP, None).gen_evaluation_key(c0, c1))
    out.append(("evk_crp", fnv(key(zero, crp)), src.pos, crs.pos))
    out.append(("evk_share", fnv(key(MR.EvaluationKeyGenProtocol(oQ, oP, src, **kw).gen_share(sk[0], sk, crp, lq, lp), zero)), src.pos, 0))
    out.append(("gal_share", fnv(key(MR.GaloisKeyGenProtocol(oQ, oP, src, **kw).gen_share(sk, 5, crp, lq, lp), zero)), src.pos, 0))
    rk = MR.RelinearizationKeyGenProtocol(oQ, oP, src, **kw)
    eph, r1 = rk.gen_share_round_one(sk, crp, lq, lp)
    out.append(("rkg_r1", fnv(MR.gadget_image(r1), eph[0], eph[1]), src.pos, 0))
    r2 = rk.gen_share_round_two(eph, sk, r1, lq, lp)
    out.append(("rkg_r2", fnv(MR.gadget_image(r2)), src.pos, 0))
    out.append(("rlk", fnv(KR.image(rk.gen_relinearization_key(r1, r2))), src.pos, 0))
    c1 = np.array(R.uniform_read(crs, N, Q), dtype=np.uint64)
    sigma, bound = MR.cks_noise(NOISE_FRESH_SK, NOISE_SIGMA)
    out.append(("cks_share", fnv(MR.KeySwitchProtocol(oQ, src, sigma, bound, **kw).gen_share(sk[0], eph[0], c1, lq, True)), src.pos, crs.pos))
    (pk0, pk1), = kg.enc.encrypt_zero_sk([sk], lq, lp, 1, 1)
    out.append(("pk", fnv(pk0[0], pk0[1], pk1[0], pk1[1]), src.pos, 0))
    pc = MR.PublicKeySwitchProtocol(oQ, oP, src, noise, sigma, bound, **kw)
    s0, s1 = pc.gen_share(sk, (pk0, pk1), c1, lq, True, False)
    out.append(("pcks_share", fnv(s0, s1), src.pos, noise.pos))
    return out


def main():
    base = answers()
    for ulps in (4, -4):
        assert answers(R.shifted(math.exp, ulps), R.shifted(R._log, ulps)) == base, ulps
    print("// generated from tests/multiparty_ref.py by tests/cpp/gen_multiparty_kat_inc.py -- do not edit")
    print(f"static const int kKatLogN = {LOGN};")
    print(f"static const uint64_t kKatSeed = {SEED:#x}ull;")
    print(f"static const double kKatNoiseSigma = {NOISE_SIGMA!r}, kKatNoiseFreshSK = {NOISE_FRESH_SK!r};")
    print("static const std::vector<uint64_t> kKatQ = {" + ", ".join(f"{q:#x}ull" for q in Q) + "}, kKatP = {" + ", ".join(f"{p:#x}ull" for p in P) + "};")
    print("struct KatAnswer { const char *name; uint64_t sum, pos, pos2; };")
    print("static const KatAnswer kKat[] = {" + ", ".join(f'{{"{n}", {s:#x}ull, {p}ull, {p2}ull}}' for n, s, p, p2 in base) + "};")


if __name__ == "__main__":
    main()
