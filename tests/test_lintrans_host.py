"""include/hering_lintrans.h on the host (no device): the three index entries against the Python restatements of the driver and
the oracle, the launch plan (csrc/lintrans_plan.h through he_debug_lintrans_plan) against a restatement here, the plan header as
a stand-alone program under the sanitizers, and a CKKS matrix-vector product end to end on the oracle with real keys."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
from drivers import lintrans as LT
from lattigo_amd import _lib
from oracle import circuits as OC
from oracle import oracle as O
from tests.bootstrap_fixtures import encode_diag_qp
from tests.rlwe_fixtures import SecretKey, ckks_decrypt, ckks_encrypt, gen_galois_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


def ints(v):
    return (C.c_int * max(len(v), 1))(*[int(x) for x in v])


# ---- the diagonal sets -----------------------------------------------------------------------------------------------------------------
CIRCUIT_SETS = [([0, 1, 2, 5], 512), ([1, 3, 130], 512), ([0, 1, 2, 3, 4, 5, 6, 7], 512), ([1, 2, 9, 17, 18], 512), ([3, 4, 5], 2048),
                (list(range(16)), 512), ([0, 2, 4, 6, 9, 11, 33], 512), ([1, 2, 3, 4, 5, 6, 7, 8, 9], 512)]


def c5_sets():
    """the DFT factors of tools/bootstrap_c5_shape.py: {j * stride mod n : |j| < 2^k}, n = 2^15"""
    n = 1 << 15
    return [(sorted({(j * (1 << s)) % n for j in range(-(1 << k) + 1, 1 << k)}), n)
            for k, s in [(4, 11), (4, 7), (4, 3), (3, 0), (5, 0), (5, 5), (5, 10)]]


def random_sets():
    rng = np.random.default_rng(20240)
    out = []
    for logs in (4, 7, 10):
        for cnt in (1, 3, 9, 40):
            out.append((sorted({int(x) for x in rng.integers(-(1 << logs), 1 << logs, size=cnt)}), 1 << logs))
    return out


ONE_GIANT = [([0, 1, 2, 3], 64), ([5], 64), ([16, 17, 19], 64)]
ONE_BABY = [([0, 8, 16, 24], 64), ([3, 11, 35], 64), ([0], 8)]
ALL_SETS = CIRCUIT_SETS + c5_sets() + random_sets() + ONE_GIANT + ONE_BABY + [([], 16), ([-1, -5, 3], 16)]


def lib_bsgs_index(lib, diags, slots, N1):
    n = len(diags)
    cap = max(min(n, slots), 1)
    r1, r2, idx, n1, n2 = (C.c_int * cap)(), (C.c_int * cap)(), (C.c_int * max(2 * n, 1))(), C.c_int(), C.c_int()
    _lib.check(lib.he_lintrans_bsgs_index(ints(diags), n, slots, N1, r1, C.byref(n1), r2, C.byref(n2), idx))
    index = {}
    for k in range(n):
        index.setdefault(idx[2 * k], []).append(idx[2 * k + 1])
    return {j: sorted(v) for j, v in index.items()}, list(r1[: n1.value]), list(r2[: n2.value])


def lib_ratio(lib, diags, maxN, logr):
    out = C.c_int()
    _lib.check(lib.he_lintrans_find_best_bsgs_ratio(ints(diags), len(diags), maxN, logr, C.byref(out)))
    return out.value


@pytest.mark.parametrize("case", range(len(ALL_SETS)))
def test_index_entries_against_the_restatements(lib, case):
    diags, slots = ALL_SETS[case]
    N1 = 1
    while N1 <= slots:
        got = lib_bsgs_index(lib, diags, slots, N1)
        for want in (LT.BSGSIndex(diags, slots, N1), OC.BSGSIndex(diags, slots, N1)):
            assert got[0] == {j: sorted(v) for j, v in want[0].items()} and got[1] == list(want[1]) and got[2] == list(want[2]), N1
        N1 <<= 1
    for logr in range(4):
        assert lib_ratio(lib, diags, slots, logr) == LT.FindBestBSGSRatio(diags, slots, logr), logr


def test_ratio_comparisons_with_a_zero_count(lib):
    """nbN1 = 0 makes the ratio +Inf (returns N1 / 2, which is 0 at N1 = 1) or NaN (compares false twice: the walk goes on)"""
    assert lib_ratio(lib, [0, 1, 2, 3], 64, 0) == LT.FindBestBSGSRatio([0, 1, 2, 3], 64, 0)
    assert lib_ratio(lib, [5], 64, 2) == LT.FindBestBSGSRatio([5], 64, 2) == 1       # 0 / 0 at every N1
    assert lib_ratio(lib, [0, 1], 2, 0) == LT.FindBestBSGSRatio([0, 1], 2, 0)        # one step of the walk
    assert lib_ratio(lib, [], 16, 1) == LT.FindBestBSGSRatio([], 16, 1)              # (-1) / (-1) = 1
    assert lib_ratio(lib, [0, 4, 8, 12], 16, 0) == LT.FindBestBSGSRatio([0, 4, 8, 12], 16, 0)


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
def plan_words(diags, slots, N1, G, nth):
    """restatement of lintrans::build_plan + plan_words (csrc/lintrans_plan.h) on reduced, distinct diagonals"""
    pos = {d: k for k, d in enumerate(diags)}
    gal = lambda r: pow(5, r & (nth - 1), nth)
    if N1 == 0:
        rots = sorted(d for d in diags if d != 0)
        return [0, len(rots), pos.get(0, -1)] + [gal(r) for r in rots]
    index, rotN1, rotN2 = LT.BSGSIndex(diags, slots, N1)
    groups = [rotN1[k: k + G] for k in range(0, len(rotN1), G)]
    w = [len(groups), len([r for r in rotN2 if r]) + len([r for r in rotN1 if r])]
    for members in groups:
        babies = sorted(set().union(*[index[j] for j in members]))
        w += [len(members), len(babies)] + members + babies
        for i in babies:
            w += [pos[j + i] if i in index[j] else -1 for j in members]
    return w + [gal(r) for r in rotN2 if r] + [gal(r) for r in rotN1 if r]


def lib_plan(lib, diags, slots, N1, G, nth):
    n_words = C.c_size_t()
    _lib.check(lib.he_debug_lintrans_plan(nth, slots, N1, G, len(diags), ints(diags), None, 0, C.byref(n_words)))
    out = (C.c_int64 * n_words.value)()
    _lib.check(lib.he_debug_lintrans_plan(nth, slots, N1, G, len(diags), ints(diags), out, n_words.value, C.byref(n_words)))
    return list(out)


PLAN_CASES = [([0, 1, 2, 3, 8, 9, 17, 18, 26, 35, 41], 8, "six giant steps: a last group that is not full at G = 4"),
              ([0, 8, 16, 24, 32], 8, "five giant steps: a last group of one at G = 2 and at G = 4"),
              ([1, 2, 9, 17, 18], 8, "a member without a baby step another member has"),
              ([5, 6, 13, 14], 8, "no i = 0 term"), ([1, 2, 3], 4, "only j = 0"), ([0], 4, "the zero diagonal alone"),
              (list(range(70)), 128, "more than 64 baby steps in one giant step"),
              (list(range(0, 300, 3)), 128, "more than 64 terms in a group, three giant steps"),
              ([0, 1, 2, 5], 0, "naive, with the zero diagonal"), ([1, 3, 130], 0, "naive, without it")]


@pytest.mark.parametrize("G", [1, 2, 4])
@pytest.mark.parametrize("case", range(len(PLAN_CASES)))
def test_plan_against_the_restatement(lib, case, G):
    diags, N1, _ = PLAN_CASES[case]
    for slots, nth in ((512, 2048), (512, 4096)):  # the second: a conjugate-invariant ring of the same degree (NthRoot = 4N)
        assert lib_plan(lib, diags, slots, N1, G, nth) == plan_words(diags, slots, N1, G, nth)


def test_plan_and_galois_elements_of_the_c5_factors(lib):
    nth = 1 << 17
    for diags, n in c5_sets():
        N1 = LT.FindBestBSGSRatio(diags, n, 1)
        assert lib_ratio(lib, diags, n, 1) == N1
        for G in (1, 2, 4):
            assert lib_plan(lib, diags, n, N1, G, nth) == plan_words(diags, n, N1, G, nth)
        # what the call asks the key set for: GaloisElements of the reference less the identity (rotation 0 needs no key)
        w = lib_plan(lib, diags, n, N1, 1, nth)
        want = sorted(set(LT.GaloisElements(nth, diags, n, 1)) - {1})
        assert sorted(w[len(w) - w[1]:]) == want
        # (he_lintrans_galois_elements takes an evaluator for its ring, which needs a context: tests/test_gpu_lintrans.py)
        assert sorted(set(pow(5, r, nth) for r in set(sum(LT.BSGSIndex(diags, n, N1)[1:], []))) - {1}) == want


def test_plan_rejects_what_it_cannot_serve(lib):
    n_words = C.c_size_t()
    bad = [([1, 1], 512, 4, 1), ([600], 512, 4, 1), ([-1], 512, 4, 1), ([1], 500, 4, 1), ([1], 512, 3, 1), ([1], 512, 4, 3 + 2), ([1], 512, 4, 0)]
    for diags, slots, N1, G in bad:
        assert lib.he_debug_lintrans_plan(2048, slots, N1, G, len(diags), ints(diags), None, 0, C.byref(n_words)) == -1, (diags, slots, N1, G)


@pytest.mark.parametrize("san", [False, True], ids=["plain", "asan-ubsan"])
def test_plan_header_as_a_program(tmp_path, san):
    exe = tmp_path / "lintrans_plan_test"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if san else ["-O2"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-I", os.path.join(ROOT, "lattigo_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "lintrans_plan_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout and " 0 failed" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


# ---- the boundary's host side --------------------------------------------------------------------------------------------------------
def test_header_symbols_and_replay_numbers(lib):
    src = open(os.path.join(ROOT, "include", "hering_lintrans.h")).read()
    import re
    mine = sorted(set(re.findall(r"\b(he_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert mine == ["he_lintrans_bsgs_index", "he_lintrans_create", "he_lintrans_destroy", "he_lintrans_evaluate", "he_lintrans_evaluate_many",
                    "he_lintrans_find_best_bsgs_ratio", "he_lintrans_galois_elements", "he_lintrans_set_group"]
    assert all(s in _lib.declared_symbols() and hasattr(lib, s) for s in mine + ["he_debug_lintrans_plan"])
    last = max(v[0] for v in _lib._TRACE_FNS_BFV.values())
    assert sorted(v[0] for v in _lib._TRACE_FNS_LINTRANS.values()) == [last + 1, last + 2]
    assert set(_lib._TRACE_FNS_LINTRANS) == {"he_lintrans_evaluate", "he_lintrans_evaluate_many"}
    names = [lib.he_prof_kernel_name(i).decode() for i in range(64)]
    assert names[names.index("rlk_finalize") + 1] == "diag_mac_group"  # appended: earlier tests index the table


# ---- end to end on the oracle ----------------------------------------------------------------------------------------------------------
def encode_restated(diagonals, N, scale, levelQ, ringQ, ringP, N1):
    """lintrans.Encode (lintrans.go:205-292) restated: in the BSGS form the diagonal of giant step j is rotated by -j (to the left
    by -j mod slots) before it is embedded"""
    n = N // 2
    sub = O.Ring(N, ringQ.moduli[: levelQ + 1])
    Vec = {}
    if N1 == 0:
        for k, d in diagonals.items():
            Vec[k % n] = encode_diag_qp(d, N, scale, sub, ringP)
    else:
        index, _, _ = OC.BSGSIndex(list(diagonals), n, N1)
        for j in index:
            rot = -j & (n - 1)
            for i in index[j]:
                Vec[j + i] = encode_diag_qp(np.roll(diagonals[j + i], -rot), N, scale, sub, ringP)
    return OC.LinearTransformation(Vec, levelQ, len(ringP.moduli) - 1, n, N1)


@pytest.mark.parametrize("N1", [0, 4])
def test_ckks_matrix_vector_end_to_end_on_the_oracle(N1):
    """logN 9, Q = [55, 45, 45], P = [55]; a real matrix with the diagonals 0, 1, 2, 5, 9 (entries in [-1, 1]) times an encrypted
    vector: encrypt, EvaluateMany, decrypt, decode, against the numpy product.  Precision reached (-log2 of the largest slot
    error, result at scale 2^45 * 2^45 before any rescale): 33.97 bits in the naive form, 34.24 bits in the BSGS form (seed 77);
    the bound is the recorded value less a 2-bit margin for seed variation."""
    recorded = {0: 33.97, 4: 34.24}[N1]
    logN = 9
    N, n = 1 << logN, 1 << (logN - 1)
    q, p = O.GenModuli(logN + 1, [55, 45, 45], [55])
    rQ, rP = O.Ring(N, q), O.Ring(N, p)
    rng = np.random.default_rng(77)
    sk = SecretKey(rng, rQ, rP)
    diagonals = {k: rng.uniform(-1, 1, n) for k in (0, 1, 2, 5, 9)}
    scale = float(1 << 45)
    olt = encode_restated(diagonals, N, scale, 2, rQ, rP, N1)
    rots = list(diagonals) if N1 == 0 else sum(OC.BSGSIndex(list(diagonals), n, N1)[1:], [])
    gks = gen_galois_keys(rng, rQ, rP, sk, [OC.GaloisElement(2 * N, r) for r in rots if r])
    z = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
    ct = ckks_encrypt(rng, rQ, sk, z, scale)
    (res,) = OC.LinTransEvaluator(O.Evaluator(rQ, rP), gks).EvaluateMany(ct, [olt])
    got = ckks_decrypt(rQ, res, sk, scale * scale)
    want = sum(d * np.roll(z, -k) for k, d in diagonals.items())
    bits = -math.log2(float(np.max(np.abs(got - want))))
    print(f"N1 = {N1}: precision reached {bits:.2f} bits")
    assert bits >= recorded - 2.0, bits
