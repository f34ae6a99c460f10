"""ckks::Evaluator of the compiled mirror include/hering.hpp: tests/cpp/ckks_evaluator_parity.cpp runs each entry of
include/hering_ckks_evaluator.h once at logN 10 on words from a file; the words it writes are held against known answers made from
tests/ckks_evaluator_ref.py over the oracle's ring primitives and key switch."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
from oracle import oracle as O
from tests import ckks_evaluator_ref as REF
from tests.conftest import Pi60, Qi60
from tests.helpers import rng_for, uniform_poly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "ckks_evaluator_parity")


def _build():
    """g++ only, against the header and the in-tree library (the flags of tests/cpp/Makefile's parity program)"""
    lib = os.path.join(ROOT, "lattigo_amd")
    if not os.path.exists(os.path.join(lib, "libhering.so")):
        graft.build()
    src = os.path.join(ROOT, "tests", "cpp", "ckks_evaluator_parity.cpp")
    deps = [src, os.path.join(lib, "libhering.so")] + [os.path.join(ROOT, "include", h) for h in ("hering.hpp", "hering.h", "hering_ckks_evaluator.h")]
    if os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in deps):
        return
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", EXE, "-L", lib, "-lhering",
                        "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr


def test_mirror_compiles_and_links():
    _build()
    r = subprocess.run([EXE, "--compile-only"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_each_entry_once_against_known_answers(tmp_path):
    _build()
    logN, nq, np_, B = 10, 3, 2, 2
    N, q, p = 1 << logN, Qi60[:nq], Pi60[:np_]
    rng = rng_for(14000)
    oQ, oP = O.Ring(N, q), O.Ring(N, p)
    oev = O.Evaluator(oQ, oP)
    beta = O.BaseRNSDecompositionVectorSize(nq - 1, np_ - 1)
    kq = np.stack([np.stack([uniform_poly(rng, q, N) for _ in range(2)]) for _ in range(beta)])
    kp = np.stack([np.stack([uniform_poly(rng, p, N) for _ in range(2)]) for _ in range(beta)])
    rlk = O.EvaluationKey(kq, kp)
    res = lambda: np.array([int(rng.integers(0, m)) for m in q], dtype=np.uint64)
    ratio, s0, s1, pre = res(), res(), res(), res()
    ct = lambda n, b: np.stack([np.stack([uniform_poly(rng, q, N) for _ in range(b)]) for _ in range(n)])  # [n][b][nq][N]
    a, b, pt, acc = ct(2, B), ct(3, B), ct(1, 1), ct(3, B)
    words = [np.array([logN, nq, np_, beta, B], dtype=np.uint64), np.array(q, dtype=np.uint64), np.array(p, dtype=np.uint64), kq.ravel(), kp.ravel(),
             ratio, s0, s1, pre, a.ravel(), b.ravel(), pt.ravel(), acc.ravel()]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate(words).astype(np.uint64).tofile(fin)
    r = subprocess.run(["timeout", "-k", "10", "120", EXE, str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0 and "PASS:" in r.stdout, r.stdout + r.stderr
    got = np.fromfile(fout, dtype=np.uint64).reshape(14, B, nq, N)
    level = nq - 1
    for e in range(B):
        A, Bc, ACC = list(a[:, e]), list(b[:, e]), list(acc[:, e])
        want = REF.ckks_add(oQ, level, True, A, Bc, 2, ratio)
        want += REF.ckks_scalar(oQ, level, 3, A, s0, s1, ACC[:2], pre)
        want += REF.ckks_mul_pt(oQ, level, A, pt[0, 0])
        want += REF.ckks_mul_pt(oQ, level, A, pt[0, 0], ACC[:2], pre)
        want += REF.ckks_mul_relin_then_add(oQ, level, A, Bc[:2], ACC)
        want += REF.ckks_mul_relin_then_add(oQ, level, A, Bc[:2], ACC[:2], pre, oev, rlk)
        assert len(want) == 14
        for i, x in enumerate(want):
            assert np.array_equal(got[i, e], x), (i, e)
