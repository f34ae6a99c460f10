"""Blind rotation on the host (no device): the library's schedule (csrc/blindrot_plan.h through he_debug_blindrot_schedule /
he_debug_blindrot_rounds) against tests/blindrot_ref.py's restatement of core/rgsw/blindrot/evaluator.go:135-280, the merger's
two properties, the restatement itself decrypting to the right signs with real keys, the plan header as a stand-alone program
(also under the host sanitizers: nothing loaded into Python is sanitized), and the boundary's mirrors."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import blindrot_ref as BR
from tests import rlwe_fixtures as F
from tests.helpers import rng_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as graft
    graft.build()
    from lattigo_amd import blindrot
    return blindrot


def _odd(rng, N, n):
    return (rng.integers(0, N, size=n) * 2 + 1).astype(np.uint64)


def _gpow(N, k):
    return pow(BR.GaloisGen, k, 2 * N)


def _rows(logN):
    """{name: row}: the cases at which the walk of the sets can go wrong"""
    N = 1 << logN
    rng = rng_for(9400 + logN)
    rows = {"random-16": _odd(rng, N, 16), "random-64": _odd(rng, N, 64), "n_lwe-1": _odd(rng, N, 1),
            "all-equal": np.full(16, _gpow(N, 37), dtype=np.uint64),
            "zero-one-minus-one": np.array([0, 1, 2 * N - 1, _gpow(N, 3), 0], dtype=np.uint64),
            # a set hit while v != 0: the negative walk leaves v = (N/2 - 1) % 10 and k = N/2 - 4 is reached three steps later
            "hit-with-pending-v": np.array([_gpow(N, N // 2 - 4)], dtype=np.uint64),
            # the tenth step of the negative walk: a hit there flushes g^9 instead of counting to 10; a hit on the eleventh
            # step follows the automorphism by g^10 directly
            "hit-on-step-10": np.array([2 * N - _gpow(N, N // 2 - 10)], dtype=np.uint64),
            "hit-on-step-11": np.array([2 * N - _gpow(N, N // 2 - 11)], dtype=np.uint64),
            "hit-at-k-1-and-minus-1": np.array([_gpow(N, 1), 2 * N - _gpow(N, 1)], dtype=np.uint64)}
    return rows


@pytest.mark.parametrize("logN", [9, 10])
def test_library_schedule_is_the_restatement(lib, logN):
    N = 1 << logN
    for name, a in _rows(logN).items():
        want = BR.schedule(N, a)
        assert lib.Schedule(logN, a) == want, name
        assert sorted(j for k, j in want if k == BR.PROD) == list(range(len(a))), name
    # the properties the cases are named for
    ops = BR.schedule(N, _rows(logN)["hit-with-pending-v"])
    pending = (N // 2 - 1) % 10 + 3
    assert 0 < pending < 10
    i = ops.index((BR.PROD, 0))
    assert ops[i - 1] == (BR.AUTO, _gpow(N, pending)) and ops[i - 2] == (BR.AUTO, 2 * N - BR.GaloisGen)
    ops = BR.schedule(N, _rows(logN)["hit-on-step-10"])
    assert ops[:2] == [(BR.AUTO, _gpow(N, 9)), (BR.PROD, 0)]
    ops = BR.schedule(N, _rows(logN)["hit-on-step-11"])
    assert ops[:2] == [(BR.AUTO, _gpow(N, 10)), (BR.PROD, 0)]
    ops = BR.schedule(N, _rows(logN)["zero-one-minus-one"])
    assert ops[-4:] == [(BR.PROD, 0), (BR.PROD, 1), (BR.PROD, 2), (BR.PROD, 4)]
    ops = BR.schedule(N, _rows(logN)["hit-at-k-1-and-minus-1"])
    assert ops[-2:] == [(BR.PROD, 0), (BR.AUTO, _gpow(N, 1))]
    i = ops.index((BR.PROD, 1))
    assert ops[i + 1] == (BR.AUTO, 2 * N - BR.GaloisGen)  # k = -1 is the last step of the negative walk and flushes nothing


def test_a_nonzero_even_word_is_einval(lib):
    from lattigo_amd import HeringError
    for a in ([2], [1, 3, 6, 5], [1, 1024 + 512]):
        with pytest.raises(HeringError) as e:
            lib.Schedule(9, a)
        assert e.value.code == EINVAL
    for a in ([2], [1, 3, 6, 5]):
        with pytest.raises(ValueError):
            BR.schedule(512, a)
    with pytest.raises(HeringError) as e:
        lib.Rounds(9, [[1, 3], [5, 4]])
    assert e.value.code == EINVAL
    assert lib.Schedule(9, [0, 1, 1023])  # zero is taken


@pytest.mark.parametrize("logN", [9, 10])
def test_merger_keeps_every_list_and_takes_the_longest_entrys_rounds(lib, logN):
    N = 1 << logN
    r = _rows(logN)
    rng = rng_for(9450 + logN)
    rows = np.stack([r["random-16"], r["all-equal"], np.concatenate([r["zero-one-minus-one"], _odd(rng, N, 11)]), _odd(rng, N, 16),
                     np.concatenate([r["hit-at-k-1-and-minus-1"], _odd(rng, N, 14)])])
    rounds = lib.Rounds(logN, rows)
    lists = [BR.schedule(N, a) for a in rows]
    for b, want in enumerate(lists):
        got = []
        for gal, prod in rounds:
            if gal[b]:
                got.append((BR.AUTO, int(gal[b])))
            if prod[b] >= 0:
                got.append((BR.PROD, int(prod[b])))
        assert got == want, b
    assert len(rounds) == max(BR.rounds_of(l) for l in lists)


def test_the_restatement_decrypts():
    """N_BR = 512 with Q = 0x7fff801, no special prime, BaseTwoDecomposition 7; N_LWE = 16 with Q = 0x3001; scales Q / 4; the
    sign test polynomial on -1 + 2 i / 8: round(8 a) / 8 == sign(v) for every v != 0"""
    rng = rng_for(9500)
    rQ, rL = O.Ring(512, [0x7FFF801]), O.Ring(16, [0x3001])
    oev = O.Evaluator(rQ, None)
    sk, skl = F.SecretKey(rng, rQ, None), F.SecretKey(rng, rL, None)
    brk, gks = BR.gen_blind_rotation_keys(rng, rQ, None, sk, skl.vals, 7)
    values = [-1 + 2 * i / 8 for i in range(8)]
    scaleLWE, scaleBR = 0x3001 / 4.0, 0x7FFF801 / 4.0
    ct = BR.encrypt_lwe_values(rng, rL, skl, values, scaleLWE)
    tp = BR.init_test_polynomial(BR.sign, scaleBR, rQ, -1, 1)
    for ntt_flag in (True, False):
        res = BR.evaluate(oev, rL, ct, {i: tp for i in range(8)}, brk, gks, ntt_flag)
        for i, v in enumerate(values):
            a = BR.decode(rQ, res[i], sk, scaleBR, is_ntt=ntt_flag)
            print(i, v, a)
            if v != 0:
                assert round(a * 8) / 8 == BR.sign(v), (i, v, a)


@pytest.mark.parametrize("san", [False, True], ids=["plain", "asan-ubsan"])
def test_plan_header_as_a_program(tmp_path, san):
    exe = tmp_path / "blindrot_plan_test"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if san else ["-O2"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + ["-I", os.path.join(ROOT, "lattigo_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "blindrot_plan_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout and " 0 failed" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


# ---- the boundary's host side --------------------------------------------------------------------------------------------
def test_header_symbols_exported(lib):
    from lattigo_amd import _lib
    L = _lib.load()
    want = ["he_galois_keyset_create", "he_galois_keyset_destroy", "he_automorphism_ct_select", "he_blind_rotate_core",
            "he_debug_blindrot_schedule", "he_debug_blindrot_rounds"]
    syms = _lib.declared_symbols()
    assert all(s in syms for s in want), "include/hering_blindrot.h is not among the declared headers"
    assert all(hasattr(L, s) for s in want)


def test_go_shim_defines_the_entries():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_go_abi.py")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    src = open(os.path.join(ROOT, "go", "hering", "blindrot.go")).read()
    for name in ("he_galois_keyset_create", "he_galois_keyset_destroy", "he_automorphism_ct_select", "he_blind_rotate_core"):
        assert "C." + name + "(" in src, name
    for method in ("BlindRotateCore", "AutomorphismSelect", "NewGaloisKeySet"):
        assert "func " in src and method in src, method


def test_cpp_mirror_compiles(tmp_path):
    """include/hering.hpp's blindrot:: wrappers type-check against hering_blindrot.h"""
    src = tmp_path / "blindrot_mirror.cpp"
    src.write_text(
        '#include "hering.hpp"\n'
        "void f(hering::rgsw::Evaluator &ev, hering::Ciphertext &acc, hering::blindrot::MemBlindRotationEvaluationKeySet &brk,\n"
        "       const std::vector<uint64_t> &a, const std::vector<int32_t> &sel, hering::Ciphertext &out) {\n"
        "    hering::blindrot::Evaluator br(ev);\n"
        "    br.BlindRotateCore(a, 16, acc, brk);\n"
        "    hering::blindrot::AutomorphismSelect(ev, acc, brk.galois, sel, out);\n"
        "}\n")
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
