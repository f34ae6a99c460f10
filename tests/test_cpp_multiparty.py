"""The multiparty protocols through the compiled mirror include/hering.hpp (namespace multiparty): tests/cpp/multiparty_mirror.cpp
compiles against the header and, on a GPU, generates one party's shares of every protocol from deterministic sources; the checksum
of each and the positions of the sources after each are the known answers of the restatement of the reference
(tests/cpp/gen_multiparty_kat_inc.py writes them into an include file)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
EXE = os.path.join(CPP, "multiparty_mirror")
INC = os.path.join(CPP, "multiparty_kat.inc")


def _build():
    """the known answers, then g++ only, against the header and the in-tree library (the flags of tests/cpp/Makefile's parity program)"""
    lib = os.path.join(ROOT, "lattigo_amd")
    assert os.path.exists(os.path.join(lib, "libhering.so")), "libhering.so not built"
    src, gen = os.path.join(CPP, "multiparty_mirror.cpp"), os.path.join(CPP, "gen_multiparty_kat_inc.py")
    refs = [gen] + [os.path.join(ROOT, "tests", f) for f in ("multiparty_ref.py", "keygen_ref.py", "encryptor_ref.py", "sampler_ref.py")]
    if not (os.path.exists(INC) and all(os.path.getmtime(INC) >= os.path.getmtime(d) for d in refs)):
        r = subprocess.run([sys.executable, gen], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        with open(INC, "w") as f:
            f.write(r.stdout)
    deps = [src, INC, os.path.join(lib, "libhering.so")] + [os.path.join(ROOT, "include", h) for h in ("hering.hpp", "hering.h", "hering_sampler.h",
                                                                                                     "hering_encryptor.h", "hering_keygen.h",
                                                                                                     "hering_multiparty.h")]
    if os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in deps):
        return
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), src, "-o", EXE, "-L", lib, "-lhering",
                        "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr


def test_multiparty_mirror_program_compiles_and_refuses_to_run_without_a_device():
    _build()
    r = subprocess.run([EXE, "--compile-only"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    import lattigo_amd as la
    if la.device_count() == 0:
        r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "FAIL:" in r.stderr and "PASS" not in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_multiparty_mirror_matches_the_restatement():
    _build()
    r = subprocess.run(["timeout", "-k", "10", "120", EXE], capture_output=True, text=True)
    assert r.returncode == 0 and "PASS:" in r.stdout, r.stdout + r.stderr
