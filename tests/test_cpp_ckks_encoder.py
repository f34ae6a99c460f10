"""ckks.Encoder through the compiled mirror include/hering.hpp (namespace ckks): tests/cpp/ckks_encoder_mirror.cpp runs FFT, IFFT,
Encode, EncodeQP and Decode on values this test writes, and its results are compared word for word with the Python mirror's on
the same device (which tests/test_gpu_ckks_encoder.py holds against the restatement of the reference)."""
import os
import subprocess

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd import ckks
from tests.gpu_common import ctx  # noqa: F401
from tests.helpers import rng_for
from tests.rlwe_fixtures import downstream_primes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "ckks_encoder_mirror")


def _build():
    """g++ only, against the header and the in-tree library (the flags of tests/cpp/Makefile's parity program)"""
    lib = os.path.join(ROOT, "lattigo_amd")
    assert os.path.exists(os.path.join(lib, "libhering.so")), "libhering.so not built"
    src = os.path.join(ROOT, "tests", "cpp", "ckks_encoder_mirror.cpp")
    deps = [src, os.path.join(lib, "libhering.so")] + [os.path.join(ROOT, "include", h) for h in ("hering.hpp", "hering.h", "hering_ckks_encoder.h")]
    if os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in deps):
        return
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", EXE, "-L", lib, "-lhering",
                        "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr


def test_ckks_encoder_mirror_program_compiles_and_links():
    _build()
    r = subprocess.run([EXE, "--compile-only"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_ckks_encoder_mirror_matches_the_python_mirror(ctx, tmp_path):
    _build()
    logN, nq, np_, log_slots, batch, scale = 9, 2, 1, 7, 2, 2.0 ** 40
    N, slots = 1 << logN, 1 << log_slots
    pr = downstream_primes(55, 4 * N, nq + np_)
    q, p = pr[:nq], pr[nq:]
    rng = rng_for(9960)
    z = rng.uniform(-1, 1, (batch, slots)) + 1j * rng.uniform(-1, 1, (batch, slots))
    words = [np.array([logN, nq, np_, log_slots, batch], dtype=np.uint64), np.array([scale]).view(np.uint64), np.array(q + p, dtype=np.uint64),
             np.ascontiguousarray(z).view(np.float64).view(np.uint64).ravel()]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate(words).astype(np.uint64).tofile(fin)
    r = subprocess.run(["timeout", "-k", "10", "240", EXE, str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0 and "PASS:" in r.stdout, r.stdout + r.stderr
    got = np.fromfile(fout, dtype=np.uint64)
    # the same calls through the Python mirror
    gQ, gP = la.Ring(ctx, N, q), la.Ring(ctx, N, p)
    enc = ckks.Encoder(gQ, gP)
    f64 = lambda a: np.ascontiguousarray(a).view(np.float64).view(np.uint64).ravel()
    pt, pq, pp = la.Poly(gQ, nq, batch), la.Poly(gQ, nq, batch), la.Poly(gP, np_, batch)
    enc.Encode(z, pt, Scale=scale, LogSlots=log_slots, IsNTT=True)
    enc.EncodeQP(z, pq, pp, Scale=scale, LogSlots=log_slots)
    want = np.concatenate([f64(enc.FFT(z, log_slots)), f64(enc.IFFT(z, log_slots)), pt.download().ravel(), pq.download().ravel(),
                           pp.download().ravel(), f64(enc.Decode(pt, Scale=scale, LogSlots=log_slots))])
    assert got.shape == want.shape and np.array_equal(got, want)
