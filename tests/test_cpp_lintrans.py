"""Linear transformations through the compiled mirror include/hering.hpp (namespace lintrans): tests/cpp/lintrans_parity.cpp runs
EvaluateMany over one BSGS and one naive transformation and EvaluateSequential of the two on words this test writes; its results
are compared word for word with oracle/circuits.py::LinTransEvaluator on the same words."""
import os
import subprocess

import numpy as np
import pytest

from drivers import lintrans as LT
from oracle import circuits as OC
from oracle import oracle as O
from tests.helpers import rng_for, uniform_poly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "lintrans_parity")


def _build():
    """g++ only, against the header and the in-tree library (the flags of tests/cpp/Makefile's parity program)"""
    lib = os.path.join(ROOT, "lattigo_amd")
    assert os.path.exists(os.path.join(lib, "libhering.so")), "libhering.so not built"
    src = os.path.join(ROOT, "tests", "cpp", "lintrans_parity.cpp")
    deps = [src, os.path.join(lib, "libhering.so")] + [os.path.join(ROOT, "include", h) for h in ("hering.hpp", "hering.h", "hering_lintrans.h")]
    if os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in deps):
        return
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", EXE, "-L", lib, "-lhering",
                        "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr


def test_lintrans_parity_program_compiles_and_links():
    _build()
    r = subprocess.run([EXE, "--compile-only"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_lintrans_mirror_matches_the_oracle(tmp_path):
    _build()
    logN = 10
    N, slots, nth = 1 << logN, 1 << (logN - 1), 2 << logN
    q, p = O.GenModuli(logN + 1, [55, 45, 45], [55, 46])
    q, p = [int(x) for x in q], [int(x) for x in p]
    nq, np_ = len(q), len(p)
    rng = rng_for(9960)
    beta = O.BaseRNSDecompositionVectorSize(nq - 1, np_ - 1)
    sets = [([1, 2, 9, 17, 18], 8), ([0, 1, 2, 5], 0)]
    rots = sorted((set(sum(LT.BSGSIndex(sets[0][0], slots, 8)[1:], [])) | set(sets[1][0])) - {0})
    words = [np.array([logN, nq, np_, beta, logN - 1, len(rots)], dtype=np.uint64), np.array(q + p, dtype=np.uint64)]
    okeys = {}
    for r in rots:
        g = OC.GaloisElement(nth, r)
        kq = np.stack([np.stack([uniform_poly(rng, q, N) for _ in range(2)]) for _ in range(beta)])
        kp = np.stack([np.stack([uniform_poly(rng, p, N) for _ in range(2)]) for _ in range(beta)])
        okeys[g] = O.EvaluationKey(kq, kp)
        words += [np.array([g], dtype=np.uint64), kq.ravel(), kp.ravel()]
    olts = []
    for diags, N1 in sets:
        vec = {}
        words.append(np.array([N1, len(diags)], dtype=np.uint64))
        for d in diags:
            vec[d] = (uniform_poly(rng, q, N), uniform_poly(rng, p, N))
            words += [np.array([d], dtype=np.uint64), vec[d][0].ravel(), vec[d][1].ravel()]
        olts.append(OC.LinearTransformation(vec, nq - 1, np_ - 1, slots, N1))
    ct = np.stack([uniform_poly(rng, q, N) for _ in range(2)])
    words.append(ct.ravel())
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate(words).astype(np.uint64).tofile(fin)
    r = subprocess.run(["timeout", "-k", "10", "240", EXE, str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0 and "PASS:" in r.stdout, r.stdout + r.stderr
    got = np.fromfile(fout, dtype=np.uint64).reshape(3, 2, nq, N)
    oe = OC.LinTransEvaluator(O.Evaluator(O.Ring(N, q), O.Ring(N, p)), okeys)
    a, b = oe.EvaluateMany(ct, olts)
    (seq,) = oe.EvaluateMany(a, [olts[1]])
    assert np.array_equal(got[0], a) and np.array_equal(got[1], b) and np.array_equal(got[2], seq)
