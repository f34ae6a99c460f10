"""The CKKS bridge through the compiled mirror include/hering.hpp: tests/cpp/bridge_mirror.cpp does one RealToComplex ->
ComplexToReal round trip and the two ring maps on words this test writes, and its results are compared word for word with the
Python mirror's on the same device (which tests/test_gpu_bridge.py holds against the reference)."""
import os
import subprocess

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd import bridge as LB
from oracle import oracle as O
from tests.gpu_common import ctx  # noqa: F401
from tests.helpers import rng_for, uniform_poly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "bridge_mirror")


def _build():
    """g++ only, against the header and the in-tree library (the flags of tests/cpp/Makefile's parity program)"""
    lib = os.path.join(ROOT, "lattigo_amd")
    assert os.path.exists(os.path.join(lib, "libhering.so")), "libhering.so not built"
    src = os.path.join(ROOT, "tests", "cpp", "bridge_mirror.cpp")
    deps = [src, os.path.join(lib, "libhering.so")] + [os.path.join(ROOT, "include", h) for h in ("hering.hpp", "hering.h", "hering_bridge.h")]
    if os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in deps):
        return
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", EXE, "-L", lib, "-lhering",
                        "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr


def test_bridge_mirror_program_compiles_and_links():
    _build()
    r = subprocess.run([EXE, "--compile-only"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_bridge_mirror_round_trip_matches_the_python_mirror(ctx, tmp_path):
    _build()
    logN, nq, np_ = 11, 4, 2
    N, n = 1 << logN, 1 << (logN - 1)
    q, p = O.GenModuli(logN + 1, [50] * nq, [55] * np_)
    q, p = list(q), list(p)
    rng = rng_for(9000)
    beta = O.BaseRNSDecompositionVectorSize(nq - 1, np_ - 1)
    keys = [(np.stack([np.stack([uniform_poly(rng, q, N) for _ in range(2)]) for _ in range(beta)]),
             np.stack([np.stack([uniform_poly(rng, p, N) for _ in range(2)]) for _ in range(beta)])) for _ in range(2)]
    ct = np.stack([uniform_poly(rng, q, n) for _ in range(2)])
    words = [np.array([logN, nq, np_, beta], dtype=np.uint64), np.array(q, dtype=np.uint64), np.array(p, dtype=np.uint64)]
    for kq, kp in keys:
        words += [kq.ravel(), kp.ravel()]
    words.append(ct.ravel())
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate(words).astype(np.uint64).tofile(fin)
    r = subprocess.run([EXE, str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PASS:" in r.stdout, r.stdout + r.stderr
    got = np.fromfile(fout, dtype=np.uint64)
    # the same calls through the Python mirror
    gQ, gP, gci = la.Ring(ctx, N, q), la.Ring(ctx, N, p), la.Ring(ctx, n, q, conjugate_invariant=True)
    gev = la.Evaluator(gQ, gP)
    sw = LB.DomainSwitcher(gev, gev.NewEvaluationKey(*keys[0]), gev.NewEvaluationKey(*keys[1]))
    real = [la.Poly(gci, nq).upload(ct[k]) for k in range(2)]
    cplx, back, un, fo = [la.Poly(gQ, nq) for _ in range(2)], [la.Poly(gci, nq) for _ in range(2)], la.Poly(gQ, nq), la.Poly(gci, nq)
    sw.RealToComplex(real, cplx)
    sw.ComplexToReal(cplx, back)
    gQ.UnfoldConjugateInvariantToStandard(real[0], un)
    gci.FoldStandardToConjugateInvariant(un, fo)
    want = np.concatenate([x.get().ravel() for x in cplx + back + [un, fo]])
    assert got.shape == want.shape and np.array_equal(got, want)
    # ... and the ring maps' known words: Unfold is the input and its mirror image, Fold(Unfold(x)) = 2 x mod q
    assert np.array_equal(un.get(), np.concatenate([ct[0], ct[0][:, ::-1]], axis=1))
    assert np.array_equal(fo.get(), O.Ring(n, q, True).binop("Add", ct[0], ct[0]))
