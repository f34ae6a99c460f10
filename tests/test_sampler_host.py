"""The restatement of the reference's samplers (tests/sampler_ref.py) held against definitions, the streams of the GPU tests
(tests/sampler_streams.py) held against their conditions, and the host accessors of include/hering_sampler.h.  No GPU."""
import math
import os
import re
from collections import deque

import numpy as np
import pytest

import __graft_entry__ as graft
from lattigo_amd import _lib
from tests import sampler_ref as R
from tests import sampler_streams as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the reference's source tree, where there is one: $HERING_REFERENCE, or a checkout named `reference` beside this repository
REFERENCE = os.environ.get("HERING_REFERENCE") or os.path.join(os.path.dirname(ROOT), "reference")
GAUSSIAN_GO = os.path.join(REFERENCE, "ring", "sampler_gaussian.go")
HEADER = os.path.join(ROOT, "include", "hering_sampler.h")


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


# ---- the library's host accessors ------------------------------------------------------------------------------------------------
def test_header_symbols_exported_and_left_out_of_recordings(lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    mine = sorted(set(re.findall(r"\b(he_[a-z0-9_]+)\s*\(", src)))
    assert len(mine) == 10 and all(s in _lib.declared_symbols() and hasattr(lib, s) for s in mine), mine
    tables = (_lib._TRACE_FNS, _lib._TRACE_FNS_RGSW, _lib._TRACE_FNS_BLINDROT, _lib._TRACE_FNS_BRIDGE, _lib._TRACE_FNS_BFV)
    reads = {"he_sampler_uniform_read", "he_sampler_gaussian_read", "he_sampler_ternary_read", "he_debug_sampler_ternary_words"}
    for s in mine:
        assert not any(s in t for t in tables), s  # no replay numbers
        assert (s in _lib._TRACE_IGNORE) == (s not in reads), s  # a Read carries host data: it fails a recording


def test_generated_tables_equal_the_construction(lib):
    from lattigo_amd import sampling
    kn, wn, fn = sampling.GaussianTables()
    assert np.array_equal(kn, R.KN) and wn.tobytes() == R.WN.tobytes() and fn.tobytes() == R.FN.tobytes()


@pytest.mark.skipif(not os.path.exists(GAUSSIAN_GO), reason="no reference source tree to read the tables from")
def test_generated_tables_equal_the_reference(lib):
    from lattigo_amd import sampling
    src = open(GAUSSIAN_GO).read()

    def table(name):
        body = re.search(r"var %s = \[128\]\w+\{(.*?)\}" % name, src, re.S).group(1)
        return [t.strip() for t in body.replace("\n", " ").split(",") if t.strip()]
    kn, wn, fn = sampling.GaussianTables()
    assert [int(t, 16) for t in table("kn")] == [int(x) for x in kn]
    assert np.array([float(t) for t in table("wn")], dtype=np.float32).tobytes() == wn.tobytes()
    assert np.array([float(t) for t in table("fn")], dtype=np.float32).tobytes() == fn.tobytes()


@pytest.mark.parametrize("P", [2 / 3, 0.25, 0.9, 1 / 3, 0.01, 0.999])
def test_ternary_matrix_words(lib, P):
    from lattigo_amd import sampling
    assert np.array_equal(sampling.TernaryMatrix(P), np.array(R.ternary_matrix(1 - P), dtype=np.uint8))


def test_refusals_without_a_device(lib):
    import ctypes as C
    assert lib.he_ternary_matrix_host(1.0, (C.c_uint64 * 2)()) == -1 and lib.he_ternary_matrix_host(0.0, (C.c_uint64 * 2)()) == -1
    h = C.c_uint64()
    assert lib.he_prng_create_callback(_lib.PRNG_READ_FN(), None, C.byref(h)) == -1
    assert lib.he_prng_create_system(C.byref(h)) == 0
    pos = (C.c_uint64 * 2)(7, 7)
    assert lib.he_prng_position(h, pos) == 0 and list(pos) == [0, 0]
    assert lib.he_prng_destroy(h) == 0 and lib.he_prng_destroy(h) == -2


# ---- the uniform restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moduli", [[65537], [576460752303439873, 65537, 0x1fffffffffe00001]])
@pytest.mark.parametrize("N", [16, 128, 512])
def test_uniform_restatement_is_the_rejection_loop(moduli, N):
    src, plain = R.seeded_source(7), R.seeded_source(7)
    got = R.uniform_read(src, N, moduli)
    words = (int.from_bytes(plain.read(8), "big") for _ in iter(int, 1))
    want = []
    for q in moduli:
        limb = []
        while len(limb) < N:
            w = next(words) & ((1 << (q - 1).bit_length()) - 1)
            if w < q:
                limb.append(w)
        want.append(limb)
    assert got == want
    assert src.pos == -(-plain.pos // 1024) * 1024  # whole 1024-byte buffers


def test_uniform_read_and_add_and_qp():
    N, mq, mp = 16, [65537, 97], [193]
    a = R.uniform_read(R.seeded_source(1), N, mq)
    s = R.seeded_source(2)
    b = R.uniform_read(R.seeded_source(2), N, mq)
    acc = R.uniform_read(s, N, mq, [list(x) for x in a])
    assert acc == [[(x + y) % q for x, y in zip(la, lb)] for la, lb, q in zip(a, b, mq)]
    s = R.seeded_source(3)
    q, p = R.uniform_read_qp(s, N, mq, mp)
    t = R.seeded_source(3)
    assert q == R.uniform_read(t, N, mq) and p == R.uniform_read(t, N, mp) and s.pos == t.pos == 2048


# ---- frequencies -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [2 / 3, 0.25, 0.9, 0.5])
def test_ternary_frequencies(P):
    N, q = 1 << 14, 97
    pol = R.ternary_read(R.seeded_source(11), N, [q], P, False)[0]
    zeros, plus, minus = pol.count(0), pol.count(1), pol.count(q - 1)
    assert zeros + plus + minus == N
    sd = math.sqrt(N * P * (1 - P))
    assert abs(zeros - N * (1 - P)) < 6 * sd  # P(0) = 1 - P
    assert abs(plus - minus) < 6 * math.sqrt(N * P)  # the sign is a fair bit


def test_gaussian_frequencies():
    N, q, sigma = 1 << 14, (1 << 40) + 1, 3.2
    pol = R.gaussian_read(R.seeded_source(12), N, [q], sigma, 6 * sigma, False)[0]
    x = np.array([w if w < q // 2 else w - q for w in (w % q for w in pol)], dtype=np.float64)
    var = sigma * sigma + 1 / 12  # the rounding adds the variance of a uniform on a unit interval
    assert abs(x.mean()) < 6 * math.sqrt(var / N)
    assert abs((x * x).mean() - var) < 6 * var * math.sqrt(2 / N)
    assert np.abs(x).max() <= round(6 * sigma)


# ---- the streams of the GPU tests ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.GAUSS_CASES, ids=repr)
def test_gaussian_streams_do_not_depend_on_exp_log(case):
    """THE STREAM CHECK the GPU tests rest on: the restatement as it is, with exp and log 4 ulps up and 4 ulps down, returns the
    same words and consumes the same bytes (the device library documents 1 ulp for both; 4 is the margin over it)"""
    N, q = 1 << case.logN, [0x1fffffffffe00001]
    runs = []
    for ulps in (0, 4, -4):
        src = case.source()
        exp, log = (math.exp, R._log) if ulps == 0 else (R.shifted(math.exp, ulps), R.shifted(R._log, ulps))
        words = [R.gaussian_read(src, N, q, case.sigma, case.bound, False, exp=exp, log=log) for _ in range(case.batch)]
        runs.append((words, src.pos))
    assert runs[0] == runs[1] == runs[2]


def test_crafted_gaussian_stream_takes_every_exit():
    tr = R.GaussTrace()
    src = S.GAUSS["crafted-logN8"].source()
    pol = R.gaussian_read(src, 256, [97], S.SIGMA, S.BOUND, False, trace=tr)[0]
    assert pol[0] == 97 and pol[1] == 0  # c = 0: the word q itself for sign 0
    assert tr.tail == 2 and tr.wedge_accept >= 2 and tr.wedge_reject >= 1 and tr.bound_reject >= 1 and tr.longest == 6
    tr = R.GaussTrace()
    R.gaussian_read(S.GAUSS["bound-is-sigma-logN8-b3"].source(), 256, [97], S.SIGMA, S.SIGMA, False, trace=tr)
    assert tr.bound_reject > 50


def _walk_graph(m):
    """every (column, d) a walk over the matrix m can be in; returns (a restart is reachable, column 55 is reachable)"""
    seen, todo, restart, out = {(0, 0)}, deque([(0, 0)]), False, False
    while todo:
        col, d = todo.popleft()
        for bit in (0, 1):
            x = 2 * d + 1 - bit
            if x > 1:
                restart = True
                x, c = 1 - bit, 0
            else:
                c = col
            if c > 54:
                out = True
                continue
            for row in (1, 0):
                x -= m[row][c]
                if x == -1:
                    break
            else:
                if (c + 1, x) not in seen:
                    seen.add((c + 1, x))
                    todo.append((c + 1, x))
    return restart, out


@pytest.mark.parametrize("P", [2 / 3, 0.25, 0.9, 1 / 3, 0.01, 0.05, 0.95, 0.999, 1e-9, 1 - 2.0 ** -53])
def test_no_density_reaches_the_restart_or_column_55(P):
    """(1 - P) 2^56 and P 2^56 are integers that add up to 2^56: every column above the lowest one of the smaller word holds exactly
    one 1, that lowest column holds two, and a walk ends there at the latest.  So the restart on d > 1 (:283-285) and the index
    panic at column 55 cannot be reached through Ternary{P}; the GPU tests reach them with he_debug_sampler_ternary_words."""
    m = R.ternary_matrix(1 - P)
    x = [sum(b << (55 - j) for j, b in enumerate(row)) for row in m]
    assert x[0] + x[1] == 1 << 56
    assert _walk_graph(m) == (False, False)
    assert _walk_graph(R.matrix_from_words(*S.KY_WORDS_RESTART)) == (True, True)


def test_crafted_ternary_streams_do_what_they_are_for():
    tr = R.KyTrace()
    R.ternary_read(S.cat_source(S.KY_LONG_WALK, 5), 16, [97], 2 / 3, False, trace=tr)
    assert tr.longest_walk == 31 and tr.sign_from_next_byte > 0
    tr = R.KyTrace()
    src = S.cat_source(S.KY_REFILL, 5)
    R.ternary_read(src, 16, [97], 2 / 3, False, trace=tr)
    assert tr.refills == 1 and src.pos == 32
    tr = R.KyTrace()
    R.ternary_read(R.seeded_source(21), 256, [97], 0.5, False, trace=tr, words=S.KY_WORDS_RESTART)
    assert tr.restarts > 10
    with pytest.raises(R.WalkOutOfColumns):
        R.ternary_read(R.bytes_source(bytes([0xFA]), 0xFF), 16, [97], 0.5, False, words=S.KY_WORDS_RESTART)


def test_aliasing_table_covers_the_header():
    """every entry of the header with a polynomial operand has a row, with the polynomial parameters in header order; the one pair
    there is, (pol, polP), is two outputs: refused (tests/test_gpu_sampler.py::test_refusals makes the call)"""
    from tests import sampler_aliasing as A
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    entries = {}
    for m in re.finditer(r"\bint\s+(he_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        polys = [p.split()[-1] for p in m.group(2).split(",") if p.split()[:1] == ["he_handle"] and p.split()[-1].startswith("pol")]
        if polys:
            entries[m.group(1)] = polys
    assert sorted(entries) == sorted(A.ROWS)
    for name, polys in entries.items():
        assert list(A.ROWS[name].params) == polys, (name, polys)
    assert A.ROWS["he_sampler_uniform_read"].verdict("pol", "polP") == "reject"
