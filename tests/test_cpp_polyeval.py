"""Polynomial evaluation through the compiled code: tests/cpp/polyeval_plan_test.cpp runs csrc/polyeval_plan.h against closed
forms as a stand-alone host program (plain, and under the address and undefined-behaviour sanitizers); tests/cpp/polyeval_parity.cpp
runs the compiled mirror include/hering.hpp (namespace polyeval) -- its host side against known answers made from the oracle-checked
planning of lattigo_amd.polyeval, its baby steps on the device against exact integer arithmetic on the same words."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
from oracle import oracle as O
from tests.helpers import rng_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "polyeval_parity")


@pytest.mark.parametrize("san", [False, True], ids=["plain", "asan-ubsan"])
def test_plan_header_as_a_program(tmp_path, san):
    exe = tmp_path / "polyeval_plan_test"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if san else ["-O2"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-I", os.path.join(ROOT, "lattigo_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "polyeval_plan_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout and " 0 failed" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


def _build():
    """g++ only, against the header and the in-tree library (the flags of tests/cpp/Makefile's parity program)"""
    lib = os.path.join(ROOT, "lattigo_amd")
    if not os.path.exists(os.path.join(lib, "libhering.so")):
        graft.build()
    src = os.path.join(ROOT, "tests", "cpp", "polyeval_parity.cpp")
    deps = [src, os.path.join(lib, "libhering.so")] + [os.path.join(ROOT, "include", h) for h in ("hering.hpp", "hering.h", "hering_polyeval.h", "hering_debug.h")]
    if os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in deps):
        return
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", EXE, "-L", lib, "-lhering",
                        "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr


def test_mirror_host_side_against_known_answers(tmp_path):
    """no device: OptimalSplit, SplitDegree, the depth check, the plan, and the BGV scalar words of the C++ mirror against those of
    lattigo_amd.polyeval, which tests/test_polyeval_host.py holds against the oracle"""
    _build()
    from lattigo_amd import polyeval as NP
    r = subprocess.run([EXE, "--compile-only"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    t, level = 65537, 5
    q, _ = O.GenModuli(10, [55] + [45] * 7, [55])
    q = [int(x) for x in q]
    sch = NP.BGVScheme(q, t)
    rng = rng_for(9900)
    cases = [(int(rng.integers(0, t)), int(rng.integers(1, t)), int(rng.integers(1, t))) for _ in range(40)]
    cases += [(0, 3, 3), (t - 1, 3, 3), (t >> 1, 1, 2), ((t >> 1) + 1, 2, 1), (5, 7, 7)]
    tinv = [sch.tInvModQ[level] % m for m in q[: level + 1]]
    words = [t, len(q), level, len(cases)] + q + tinv + [x for c in cases for x in c]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    np.array(words, dtype=np.uint64).tofile(fin)
    r = subprocess.run([EXE, "--host", str(fin), str(fout)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "PASS:" in r.stdout, r.stdout + r.stderr
    got = [int(x) for x in np.fromfile(fout, dtype=np.uint64)]
    want = [NP.OptimalSplit(ld) for ld in range(1, 31)] + [x for n in range(1, 65) for x in NP.SplitDegree(n)]
    for c, xs, os_ in cases:
        want += sch.term(level, c, xs, os_, [])[0][0]
        want += sch.const_words(level, os_, c)[0]
    plan = NP.Plan(17, level=7)
    want += [plan.log_split, plan.depth, len(plan.leaves), len(plan.steps), plan.out_level]
    want += [x % (1 << 64) for f in plan.leaves for x in f] + [x % (1 << 64) for s in plan.steps for x in s]
    assert got == want


@pytest.mark.gpu
def test_mirror_baby_steps_on_the_device(tmp_path):
    """degree 12 on five limbs across the arithmetic classes, batch 3, every baby step in one call at G = 1 and G = 4"""
    _build()
    from lattigo_amd import polyeval as NP
    from tests import boundary as Bd
    logN, degree, B = 8, 12, 3
    N = 1 << logN
    q = Bd.class_chain(logN, "hiIdD")
    nq = len(q)
    plan = NP.Plan(degree, level=nq - 1)
    rows = sum(f[0] + 1 for f in plan.leaves)
    npow = max(f[0] for f in plan.leaves)
    rng = rng_for(9910)
    s0 = np.stack([rng.integers(0, m, size=rows, dtype=np.uint64) for m in q], axis=1)
    s1 = np.stack([rng.integers(0, m, size=rows, dtype=np.uint64) for m in q], axis=1)
    X = np.stack([np.stack([np.stack([np.stack([Bd.word_row("uniform", rng, m, N) for m in q]) for _ in range(B)]) for _ in range(2)]) for _ in range(npow)])
    words = [np.array([logN, nq, degree, B, npow] + q + [len(plan.leaves)], dtype=np.uint64), s0.ravel(), s1.ravel(), X.ravel()]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate(words).astype(np.uint64).tofile(fin)
    r = subprocess.run(["timeout", "-k", "10", "120", EXE, str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0 and "PASS:" in r.stdout, r.stdout + r.stderr
    got = np.fromfile(fout, dtype=np.uint64)
    want, row = [], 0
    half = N // 2
    for deg, lvl, _, ctdeg, present in plan.leaves:
        assert ctdeg == 1
        for c in range(2):
            acc = np.zeros((B, lvl + 1, N), dtype=object)
            for l in range(lvl + 1):
                if c == 0 and present & 1:
                    acc[:, l, :half] += int(s0[row][l])
                    acc[:, l, half:] += int(s1[row][l])
                for k in range(1, deg + 1):
                    if (present >> k) & 1:
                        acc[:, l, :half] += int(s0[row + k][l]) * X[k - 1, c, :, l, :half].astype(object)
                        acc[:, l, half:] += int(s1[row + k][l]) * X[k - 1, c, :, l, half:].astype(object)
                acc[:, l] %= q[l]
            want.append(acc.astype(np.uint64).ravel())
        row += deg + 1
    want = np.concatenate(want)
    assert got.size == 2 * want.size
    assert np.array_equal(got[: want.size], want) and np.array_equal(got[want.size:], want)


@pytest.mark.gpu
def test_mirror_evaluate_is_one_native_call_and_matches_the_oracle(tmp_path):
    """polyeval::Polynomial::Evaluate and EvaluateFromPowerBasis of the C++ mirror (BGV, degree 7, batch 2, words planned by
    lattigo_amd.polyeval) against oracle/polyeval_ref.py on the oracle backend"""
    _build()
    from lattigo_amd import polyeval as NP
    from oracle import circuits as OC
    from oracle import polyeval_ref as PR
    from tests.helpers import uniform_poly
    logN, degree, B, t = 10, 7, 2, 65537
    N = 1 << logN
    q, p = O.GenModuli(logN + 1, [55] + [45] * 5, [55, 55])
    q, p = [int(x) for x in q], [int(x) for x in p]
    nq, np_ = len(q), len(p)
    rng = rng_for(9920)
    beta = O.BaseRNSDecompositionVectorSize(nq - 1, np_ - 1)
    kq = np.stack([np.stack([uniform_poly(rng, q, N) for _ in range(2)]) for _ in range(beta)])
    kp = np.stack([np.stack([uniform_poly(rng, p, N) for _ in range(2)]) for _ in range(beta)])
    coeffs = [int(x) for x in rng.integers(1, t, size=degree + 1)]
    planned = NP.Polynomial(coeffs).Plan(NP.BGVScheme(q, t), nq - 1, 3, 11, copy_input=False)
    L = nq
    rows0 = []
    for f in planned.leaves:
        by_k = {k: s0 for k, s0, _ in f["words"]}
        for k in range(f["degree"] + 1):
            w = list(by_k.get(k, []))
            rows0.append(w + [0] * (L - len(w)))
    s0 = np.array(rows0, dtype=np.uint64)
    ct = np.stack([np.stack([uniform_poly(rng, q, N) for _ in range(B)]) for _ in range(2)])  # [2][B][nq][N]
    words = [np.array([logN, nq, np_, beta, degree, t, B] + q + p, dtype=np.uint64), kq.ravel(), kp.ravel(),
             np.array([len(planned.leaves)], dtype=np.uint64), s0.ravel(), s0.ravel(), ct.ravel()]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate(words).astype(np.uint64).tofile(fin)
    r = subprocess.run(["timeout", "-k", "10", "120", EXE, "--evaluate", str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0 and "PASS:" in r.stdout, r.stdout + r.stderr
    lv = planned.out_level
    got = np.fromfile(fout, dtype=np.uint64).reshape(2, 2, B, lv + 1, N)
    obe = OC.BGVCtEvaluator(O.Evaluator(O.Ring(N, q), O.Ring(N, p)), t, O.EvaluationKey(kq, kp))
    for b in range(B):
        want = PR.evaluate_polynomial(obe, OC.Ct([ct[0][b], ct[1][b]], 3), coeffs, 11)
        assert (want.level, want.Scale) == (lv, planned.out_scale)
        for call in range(2):
            assert np.array_equal(got[call][:, b], np.stack(want.Value)), (call, b)
