"""BFV through the compiled mirror include/hering.hpp (namespace bgv): tests/cpp/bfv_mirror.cpp runs MulRelinScaleInvariant,
MulScaleInvariant, the squaring call and Quantize on words this test writes, and its results are compared word for word with the
Python mirror's on the same device (which tests/test_gpu_bfv.py holds against the reference)."""
import os
import subprocess

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd import bfv as BFV
from oracle import oracle as O
from tests import bfv_ref as F
from tests.gpu_common import ctx  # noqa: F401
from tests.helpers import rng_for, uniform_poly
from tests.rlwe_fixtures import downstream_primes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "bfv_mirror")


def _build():
    """g++ only, against the header and the in-tree library (the flags of tests/cpp/Makefile's parity program)"""
    lib = os.path.join(ROOT, "lattigo_amd")
    assert os.path.exists(os.path.join(lib, "libhering.so")), "libhering.so not built"
    src = os.path.join(ROOT, "tests", "cpp", "bfv_mirror.cpp")
    deps = [src, os.path.join(lib, "libhering.so")] + [os.path.join(ROOT, "include", h) for h in ("hering.hpp", "hering.h", "hering_bfv.h")]
    if os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in deps):
        return
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", EXE, "-L", lib, "-lhering",
                        "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr


def test_bfv_mirror_program_compiles_and_links():
    _build()
    r = subprocess.run([EXE, "--compile-only"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_bfv_mirror_matches_the_python_mirror(ctx, tmp_path):
    _build()
    logN, t = 11, 65537
    N = 1 << logN
    q, p = O.GenModuli(logN + 1, [50] * 4, [55] * 2)
    q, p = [int(x) for x in q], [int(x) for x in p]
    nq, np_ = len(q), len(p)
    nm = F.level_qmul(q, logN)[-1] + 1
    qm = downstream_primes(61, 2 * N, nm, set(q) | set(p))
    rng = rng_for(9950)
    beta = O.BaseRNSDecompositionVectorSize(nq - 1, np_ - 1)
    kq = np.stack([np.stack([uniform_poly(rng, q, N) for _ in range(2)]) for _ in range(beta)])
    kp = np.stack([np.stack([uniform_poly(rng, p, N) for _ in range(2)]) for _ in range(beta)])
    ct0, ct1 = (np.stack([uniform_poly(rng, q, N) for _ in range(2)]) for _ in range(2))
    cM = uniform_poly(rng, qm, N)
    words = [np.array([logN, nq, np_, nm, beta, t], dtype=np.uint64), np.array(q + p + qm, dtype=np.uint64), kq.ravel(), kp.ravel(),
             ct0.ravel(), ct1.ravel(), cM.ravel()]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate(words).astype(np.uint64).tofile(fin)
    r = subprocess.run(["timeout", "-k", "10", "240", EXE, str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0 and "PASS:" in r.stdout, r.stdout + r.stderr
    got = np.fromfile(fout, dtype=np.uint64)
    # the same calls through the Python mirror
    gQ, gP, gM = la.Ring(ctx, N, q), la.Ring(ctx, N, p), la.Ring(ctx, N, qm)
    gev = la.Evaluator(gQ, gP)
    gs = BFV.ScaleInvariantEvaluator(gev, gM, t)
    rlk = gev.NewEvaluationKey(kq, kp)
    a, b = [la.Poly(gQ, nq).upload(ct0[k]) for k in range(2)], [la.Poly(gQ, nq).upload(ct1[k]) for k in range(2)]
    new = lambda n: [la.Poly(gQ, nq) for _ in range(n)]
    relin, deg2, sq = new(2), new(3), new(2)
    gs.MulRelinScaleInvariant(nq - 1, a, b, rlk, relin)
    gs.MulRelinScaleInvariant(nq - 1, a, b, None, deg2)
    gs.MulRelinScaleInvariant(nq - 1, a, a, rlk, sq)
    gs.Quantize(nq - 1, b[0], la.Poly(gM, nm).upload(cM))
    want = np.concatenate([x.get().ravel() for x in relin + deg2 + sq + [b[0]]])
    assert got.shape == want.shape and np.array_equal(got, want)
