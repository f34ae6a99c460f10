#!/usr/bin/env python3
"""Known-answer words of tests/cpp/rgsw_encryptor_mirror.cpp from the restatement of the reference (tests/rgsw_encryptor_ref.py), as
a C++ include: python gen_rgsw_encryptor_kat_inc.py > rgsw_encryptor_kat.inc.  The stream is splitmix64 of (seed + block) per 8-byte
block, which the program restates; the answers are FNV-1a checksums over the words of each result and the position of the source
after each call.  The same answers with exp / log moved 4 ulps up and down are asserted equal here, so that none depends on the
device's exp / log."""
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

import numpy as np  # noqa: E402

from oracle import oracle as O  # noqa: E402
from tests import keygen_ref as KR  # noqa: E402
from tests import rgsw_encryptor_ref as GR  # noqa: E402
from tests import sampler_ref as R  # noqa: E402
from tests.conftest import Pi60, Qi60  # noqa: E402

LOGN, Q, P, PW2, SEED = 5, Qi60[:2], Pi60[:1], 7, 0x2545F4914F6CDD1D
LOGN_LWE, Q_LWE = 4, 0x3001
SEL, M = [1, -1, 0], 2
M64 = (1 << 64) - 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def source(seed):
    def gen(off, n):
        out = bytearray()
        for o in range(off, off + n):
            out.append((splitmix64((seed + (o >> 3)) & M64) >> (8 * (o & 7))) & 0xFF)
        return bytes(out)
    return R.Source(gen)


def fnv(words, h=0xCBF29CE484222325):
    for w in np.asarray(words, dtype=np.uint64).ravel():
        h = ((h ^ int(w)) * 0x100000001B3) & M64
    return h


def plaintext(salt):
    """word j of limb i: splitmix64(salt, i, j) mod q_i, which the program restates"""
    N = 1 << LOGN
    return np.array([[splitmix64((salt << 32) + (i << 16) + j) % q for j in range(N)] for i, q in enumerate(Q)], dtype=np.uint64)


def lwe_secret():
    rl = O.Ring(1 << LOGN_LWE, [Q_LWE])
    return rl, KR.KeyGenerator(rl, None, source(SEED + 2)).gen_secret_key(0, -1)[0]


def answers(exp=math.exp, log=R._log):
    """[(name, checksum, position)] in the order the program makes its calls"""
    N = 1 << LOGN
    oQ, oP = O.Ring(N, Q), O.Ring(N, P)
    src = source(SEED)
    sk = KR.KeyGenerator(oQ, oP, src, exp=exp, log=log).gen_secret_key(len(Q) - 1, len(P) - 1)
    out = [("sk", fnv(np.concatenate([sk[0], sk[1]])), src.pos)]
    enc = GR.Encryptor(oQ, oP, src, sk, exp=exp, log=log)
    out.append(("encrypt", fnv(GR.image(enc.encrypt(plaintext(1), False, False, len(Q) - 1, len(P) - 1, PW2))), src.pos))
    out.append(("zero", fnv(GR.image(enc.encrypt_zero(len(Q) - 1, len(P) - 1, PW2))), src.pos))
    pts = np.stack([plaintext(2 + s) for s in range(M)])
    h = 0xCBF29CE484222325
    for ct in enc.encrypt_table(pts, SEL, len(Q) - 1, len(P) - 1, PW2):
        h = fnv(GR.image(ct), h)
    out.append(("table", h, src.pos))
    rl, skl = lwe_secret()
    brk, gks, _, _ = GR.gen_evaluation_key_new(oQ, oP, sk, rl, skl, len(Q) - 1, len(P) - 1, PW2, src, None, exp=exp, log=log)
    h = 0xCBF29CE484222325
    for ct in brk:
        h = fnv(GR.image(ct), h)
    for key in gks.values():
        h = fnv(KR.image(key), h)
    out.append(("blindrot", h, src.pos))
    return out


def main():
    base = answers()
    for ulps in (4, -4):
        assert answers(R.shifted(math.exp, ulps), R.shifted(R._log, ulps)) == base, ulps
    _, skl = lwe_secret()
    print("// generated from tests/rgsw_encryptor_ref.py by tests/cpp/gen_rgsw_encryptor_kat_inc.py -- do not edit")
    print(f"static const int kKatLogN = {LOGN}, kKatPw2 = {PW2}, kKatLogNLWE = {LOGN_LWE}, kKatM = {M};")
    print(f"static const uint64_t kKatSeed = {SEED:#x}ull, kKatQLWE = {Q_LWE:#x}ull;")
    print("static const std::vector<uint64_t> kKatQ = {" + ", ".join(f"{q:#x}ull" for q in Q) + "}, kKatP = {" + ", ".join(f"{p:#x}ull" for p in P) + "};")
    print("static const std::vector<int32_t> kKatSel = {" + ", ".join(str(s) for s in SEL) + "};")
    print("static const std::vector<uint64_t> kKatSkLWE = {" + ", ".join(f"{int(w):#x}ull" for w in skl[0]) + "};")
    print("struct KatAnswer { const char *name; uint64_t sum, pos; };")
    print("static const KatAnswer kKat[] = {" + ", ".join(f'{{"{n}", {s:#x}ull, {p}ull}}' for n, s, p in base) + "};")


if __name__ == "__main__":
    main()
