#!/usr/bin/env python3
"""Known-answer words of tests/cpp/keygen_mirror.cpp from the restatement of the reference (tests/keygen_ref.py), as a C++ include:
python gen_keygen_kat_inc.py > keygen_kat.inc.  The stream is splitmix64 of (seed + block) per 8-byte block, which the program
restates; the answers are FNV-1a checksums over the words of each key and the position of the source after each call.  The same
answers with exp / log moved 4 ulps up and down are asserted equal here, so that none depends on the device's exp / log."""
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

import numpy as np  # noqa: E402

from oracle import oracle as O  # noqa: E402
from tests import keygen_ref as KR  # noqa: E402
from tests import sampler_ref as R  # noqa: E402
from tests.conftest import Pi60, Qi60  # noqa: E402

LOGN, Q, P, SEED, HW = 5, Qi60[:3], Pi60[:1], 0x9E3779B97F4A7C15, 11
M64 = (1 << 64) - 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def source():
    def gen(off, n):
        out = bytearray()
        for o in range(off, off + n):
            out.append((splitmix64((SEED + (o >> 3)) & M64) >> (8 * (o & 7))) & 0xFF)
        return bytes(out)
    return R.Source(gen)


def fnv(words):
    h = 0xCBF29CE484222325
    for w in np.asarray(words, dtype=np.uint64).ravel():
        h = ((h ^ int(w)) * 0x100000001B3) & M64
    return h


def answers(exp=math.exp, log=R._log):
    """[(name, checksum, position)] in the order the program makes its calls"""
    N = 1 << LOGN
    oQ, oP = O.Ring(N, Q), O.Ring(N, P)
    src = source()
    kg = KR.KeyGenerator(oQ, oP, src, exp=exp, log=log)
    out = []
    sk = kg.gen_secret_key(len(Q) - 1, len(P) - 1)
    out.append(("sk", fnv(np.concatenate([sk[0], sk[1]])), src.pos))
    (pk0, pk1), = kg.enc.encrypt_zero_sk([sk], len(Q) - 1, len(P) - 1, 1, 1)
    out.append(("pk", fnv(np.concatenate([pk0[0], pk0[1], pk1[0], pk1[1]])), src.pos))
    out.append(("rlk", fnv(KR.image(kg.gen_relinearization_key(sk, len(Q) - 1, len(P) - 1))), src.pos))
    for g, key in zip((5, 2 * N - 1), kg.gen_galois_keys([5, 2 * N - 1], sk, len(Q) - 1, len(P) - 1)):
        out.append((f"gk{g}", fnv(KR.image(key)), src.pos))
    skh = kg.gen_secret_key_hw(HW, len(Q) - 1, len(P) - 1)
    out.append(("sk_hw", fnv(np.concatenate([skh[0], skh[1]])), src.pos))
    out.append(("evk_pw2", fnv(KR.image(kg.gen_evaluation_key(sk[0], skh, 1, 0, 20))), src.pos))
    return out


def main():
    base = answers()
    for ulps in (4, -4):
        assert answers(R.shifted(math.exp, ulps), R.shifted(R._log, ulps)) == base, ulps
    print("// generated from tests/keygen_ref.py by tests/cpp/gen_keygen_kat_inc.py -- do not edit")
    print(f"static const int kKatLogN = {LOGN}, kKatHW = {HW};")
    print(f"static const uint64_t kKatSeed = {SEED:#x}ull;")
    print("static const std::vector<uint64_t> kKatQ = {" + ", ".join(f"{q:#x}ull" for q in Q) + "}, kKatP = {" + ", ".join(f"{p:#x}ull" for p in P) + "};")
    print("struct KatAnswer { const char *name; uint64_t sum, pos; };")
    print("static const KatAnswer kKat[] = {" + ", ".join(f'{{"{n}", {s:#x}ull, {p}ull}}' for n, s, p in base) + "};")


if __name__ == "__main__":
    main()
