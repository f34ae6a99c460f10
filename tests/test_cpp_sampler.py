"""The ring samplers through the compiled mirror include/hering.hpp: tests/cpp/sampler_mirror.cpp draws a ringqp uniform polynomial, a
Gaussian one, a ternary one added to it and a ternary one of density 0.5 from the bytes this test writes, and its words and
positions are compared with the Python mirror's on the same bytes (which tests/test_gpu_sampler.py holds against the restatement
of the reference)."""
import os
import subprocess

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd import sampling
from tests import sampler_ref as R
from tests import sampler_streams as S
from tests.conftest import Pi60, Qi60
from tests.gpu_common import ctx  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "sampler_mirror")


def _build():
    """g++ only, against the header and the in-tree library (the flags of tests/cpp/Makefile's parity program)"""
    lib = os.path.join(ROOT, "lattigo_amd")
    assert os.path.exists(os.path.join(lib, "libhering.so")), "libhering.so not built"
    src = os.path.join(ROOT, "tests", "cpp", "sampler_mirror.cpp")
    deps = [src, os.path.join(lib, "libhering.so")] + [os.path.join(ROOT, "include", h) for h in ("hering.hpp", "hering.h", "hering_sampler.h")]
    if os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in deps):
        return
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", EXE, "-L", lib, "-lhering",
                        "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr


def test_sampler_mirror_program_compiles_and_links():
    _build()
    r = subprocess.run([EXE, "--compile-only"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_sampler_mirror_matches_the_python_mirror(ctx, tmp_path):
    _build()
    logN, nq, np_, batch = 8, 2, 1, 2
    N, q, p = 1 << logN, Qi60[:nq], Pi60[:np_]
    case = S.GAUSS["sequence-logN8-b3"]  # a stream that has passed the host check at this degree (read here at an offset: the
    # comparison is between two mirrors of one library, so exp / log cancel)
    nbytes = 64 * 1024
    data = case.source().read(nbytes)
    words = [np.array([logN, nq, np_, batch, nbytes], dtype=np.uint64), np.array(q + p, dtype=np.uint64), np.frombuffer(data, dtype=np.uint64)]
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate(words).astype(np.uint64).tofile(fin)
    r = subprocess.run(["timeout", "-k", "10", "240", EXE, str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0 and "PASS:" in r.stdout, r.stdout + r.stderr
    got = np.fromfile(fout, dtype=np.uint64)
    # the same calls through the Python mirror
    gQ, gP = la.Ring(ctx, N, q), la.Ring(ctx, N, p)
    prng = sampling.PRNG(R.bytes_source(data).read)
    pos = lambda: np.array([prng.Position()], dtype=np.uint64)
    uq, up = sampling.UniformSampler(prng, gQ, gP).ReadNew(batch)
    want = [uq.download().ravel(), up.download().ravel(), pos()]
    e = sampling.GaussianSampler(prng, gQ, 3.2, 19.2, True).ReadNew(batch)
    want += [e.download().ravel(), pos()]
    sampling.TernarySampler(prng, gQ, 2 / 3, True).ReadAndAdd(e)
    want += [e.download().ravel(), pos()]
    want += [sampling.TernarySampler(prng, gQ.AtLevel(0), 0.5, False).ReadNew(batch).download().ravel(), pos()]
    want = np.concatenate(want)
    assert got.shape == want.shape and np.array_equal(got, want)
