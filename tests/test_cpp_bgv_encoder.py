"""bgv.Encoder through the compiled mirror include/hering.hpp (namespace bgv): tests/cpp/bgv_encoder_mirror.cpp runs IndexMatrix,
EncodeRingT, DecodeRingT, RingT2Q, RingQ2T, Encode, EncodeQP and Decode on values this test writes, and its results are compared
word for word with the Python mirror's on the same device (which tests/test_gpu_bgv_encoder.py holds against the restatement of
the reference)."""
import os
import subprocess

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd import bgv
from tests.gpu_common import ctx  # noqa: F401
from tests.helpers import rng_for
from tests.rlwe_fixtures import downstream_primes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "bgv_encoder_mirror")


def _build():
    """g++ only, against the header and the in-tree library (the flags of tests/cpp/Makefile's parity program)"""
    lib = os.path.join(ROOT, "lattigo_amd")
    assert os.path.exists(os.path.join(lib, "libhering.so")), "libhering.so not built"
    src = os.path.join(ROOT, "tests", "cpp", "bgv_encoder_mirror.cpp")
    deps = [src, os.path.join(lib, "libhering.so")] + [os.path.join(ROOT, "include", h) for h in ("hering.hpp", "hering.h", "hering_bgv_encoder.h")]
    if os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in deps):
        return
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", EXE, "-L", lib, "-lhering",
                        "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr


def test_bgv_encoder_mirror_program_compiles_and_links():
    _build()
    r = subprocess.run([EXE, "--compile-only"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("T,logNT", [(65537, 9), (257, 7)])
def test_bgv_encoder_mirror_matches_the_python_mirror(ctx, tmp_path, T, logNT):
    _build()
    logN, nq, np_, batch, scale = 9, 2, 1, 2, 5
    N, NT = 1 << logN, 1 << logNT
    pr = downstream_primes(55, 2 * N, nq + np_)
    q, p = pr[:nq], pr[nq:]
    rng = rng_for(9970 + logNT)
    v = rng.integers(-(1 << 62), 1 << 62, (batch, NT)).astype(np.int64)
    words = [np.array([logN, logNT, nq, np_, batch, T, scale], dtype=np.uint64), np.array(q + p, dtype=np.uint64), v.view(np.uint64).ravel()]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate(words).astype(np.uint64).tofile(fin)
    r = subprocess.run(["timeout", "-k", "10", "240", EXE, str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0 and "PASS:" in r.stdout, r.stdout + r.stderr
    got = np.fromfile(fout, dtype=np.uint64)
    # the same calls through the Python mirror
    gQ, gP, gT = la.Ring(ctx, N, q), la.Ring(ctx, N, p), la.Ring(ctx, NT, [T])
    enc = bgv.Encoder(gQ, gT, gP)
    pT, back = la.Poly(gT, 1, batch), la.Poly(gT, 1, batch)
    pt, pq, pp = la.Poly(gQ, nq, batch), la.Poly(gQ, nq, batch), la.Poly(gP, np_, batch)
    want = [enc.IndexMatrix(), enc.EncodeRingT(v, scale, pT).download().ravel(), enc.DecodeRingT(pT, scale).ravel(),
            enc.RingT2Q(nq - 1, True, pT, pt).download().ravel(), enc.RingQ2T(nq - 1, True, pt, back).download().ravel(),
            enc.Encode(v, pt, Scale=scale).download().ravel()]
    enc.EncodeQP(v, pq, pp, Scale=scale, IsMontgomery=True)
    want += [pq.download().ravel(), pp.download().ravel(), enc.Decode(pt, Scale=scale, signed=True).view(np.uint64).ravel()]
    want = np.concatenate(want)
    assert got.shape == want.shape and np.array_equal(got, want)
