"""Blind rotation on the host (no device): the library's schedule (csrc/blindrot_plan.h through he_debug_blindrot_schedule /
he_debug_blindrot_rounds) against tests/blindrot_ref.py's restatement of core/rgsw/blindrot/evaluator.go:135-280, the merger's
two properties, the restatement itself decrypting to the right signs with real keys, the plan header as a stand-alone program
(also under the host sanitizers: nothing loaded into Python is sanitized), the boundary's mirrors, and the constructions of
tests/test_gpu_blindrot_edges.py (tests/blindrot_edges.py): each shape, key and row has the property it is built for."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import blindrot_edges as BE
from tests import blindrot_ref as BR
from tests import rgsw_edges as E
from tests import rgsw_ref as R
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


# ---- the constructions of tests/test_gpu_blindrot_edges.py: each has the property it is built for ----------------------------------
@pytest.mark.parametrize("name", sorted(BE.lift_shapes()))
def test_planted_galois_keys_put_the_lift_boundary_into_the_p_accumulator(name):
    """GadgetProductLazy of NTT(1) with the planted key: tests/rgsw_ref.lift_targets -- (p - 1) / 2, (p + 1) / 2, 0, p - 1 -- as the
    coefficients of one component's P accumulator and zero as the other's"""
    s = BE.lift_shapes()[name]
    assert s["pw2"] != 0 and BE.select_by_header(s)
    N = 1 << s["logN"]
    oQ, oP = O.Ring(N, s["q"]), O.Ring(N, s["p"])
    oev = O.Evaluator(oQ, oP)
    p = s["p"][0]
    for component in range(2):
        key = BE.planted_key(rng_for(9520 + component), oQ, oP, s["pw2"], component)
        _, ctP = oev.GadgetProductLazy(len(s["q"]) - 1, R.ntt_of_one(oQ, len(s["q"])), key)
        pc = np.stack([oP.INTT(oP.unop("Reduce", ctP[c])) for c in range(2)])
        assert np.array_equal(pc[component, 0], R.lift_targets(p, N)) and not pc[1 - component].any()
        assert [int(v) for v in pc[component, 0, :4]] == [(p - 1) // 2, (p + 1) // 2, 0, p - 1]


def test_select_shapes_lie_where_the_header_says():
    inside = {**BE.inside_shapes(), **BE.moduli_shapes(), **BE.lift_shapes()}
    assert all(BE.select_by_header(s) for s in inside.values())
    assert all(not BE.select_by_header(s, ci) for s, ci in BE.outside_shapes().values())
    N = lambda s: 1 << s["logN"]
    lds = lambda s: (2 * len(s["q"]) * N(s) + N(s) + N(s) // 16) * 8
    ins, out = BE.inside_shapes(), BE.outside_shapes()
    # the largest footprint of each degree fits 64 KiB and one limb more does not
    for a, b in (("9x7+P", "9x8+P"), ("10x3+P", "10x4+P"), ("11x1+P", "11x2+P")):
        assert lds(ins[a]) <= BE.LDS_BYTES < lds(out[b][0]) and len(out[b][0]["q"]) == len(ins[a]["q"]) + 1
    assert lds(ins["10x3"]) == lds(ins["10x3+P"]) and not ins["10x3"]["p"]
    shift = lambda s: (s["nj"][0] - 1) * s["pw2"]
    assert shift(ins["pw2-7-nj-10"]) == shift(ins["pw2-9-nj-8"]) == BE.LAST_SHIFT and shift(out["pw2-8-nj-9"][0]) == 64
    assert sum(R.window_counts(ins["beta255"]["q"], 1)) == 255
    assert len(out["two-P"][0]["p"]) == 2 and out["two-P"][0]["pw2"] == 0 and out["conjugate-invariant"][1]
    assert all(q % (4 << 10) == 1 for q in out["conjugate-invariant"][0]["q"] + out["conjugate-invariant"][0]["p"])
    # one destination below the mask: the 14-bit prime at a mask of 14 and of 16 bits, none at 13
    m = BE.moduli_shapes()
    assert sorted(m) == ["10-IDi", "10-hd+14|i", "11-14|D", "9-hiIdD+14|h-pw2-13", "9-hiIdD+14|h-pw2-14", "9-hiIdD+14|h-pw2-16", "9-hiIdD+14|h-pw2-61"]
    below = lambda s: [q for q in s["q"] + s["p"] if q <= (1 << s["pw2"]) - 1]
    assert below(m["9-hiIdD+14|h-pw2-14"]) == below(m["9-hiIdD+14|h-pw2-16"]) == below(m["10-hd+14|i"]) == [E.Q14]
    assert not below(m["9-hiIdD+14|h-pw2-13"]) and not below(m["11-14|D"]) and (1 << 16) - 1 >= 4 * E.Q14
    wide = m["9-hiIdD+14|h-pw2-61"]
    assert sorted(below(wide)) == sorted(wide["q"] + wide["p"]) and R.window_counts(wide["q"], 61) == [1] * 6
    assert max(wide["q"]) - 1 >= 4 * max(q for q in wide["q"] if q < (1 << 58))  # (a whole coefficient against the next class down)
    assert len(set(BE.galois_pair(512))) == 2 and all(g in BR.galois_elements(512) for g in BE.galois_pair(512))


def test_schedule_edge_rows(lib):
    logN, N = BE.ROW_LOGN, 1 << BE.ROW_LOGN
    rows = BE.rows()
    assert rows.shape == (len(BE.ROW_NAMES), BE.ROW_N_LWE) and BR.GaloisGen == 5
    lists = [BR.schedule(N, a) for a in rows]
    for name, a, want in zip(BE.ROW_NAMES, rows, lists):
        assert lib.Schedule(logN, a) == want, name
    assert lists[0] == lists[1] == lists[2]
    prods = [(BR.PROD, j) for j in range(BE.ROW_N_LWE)]
    assert lists[0][-BE.ROW_N_LWE:] == prods, "set 0 is served by the last line of BlindRotateCore"
    # (the negative walk's 255 steps leave v = 5 pending: the positive walk's first set flushes g^5 before its products)
    i = lists[3].index((BR.AUTO, 2 * N - 5))
    assert lists[3][i + 1:i + 2 + BE.ROW_N_LWE] == [(BR.AUTO, pow(5, 5, 2 * N))] + prods, "the first step of the positive walk"
    assert lists[4][:BE.ROW_N_LWE] == prods, "the first step of the negative walk"
    assert lists[5][-BE.ROW_N_LWE - 1:] == prods + [(BR.AUTO, 5)], "k = 1: the last step of the positive walk"
    i = lists[6].index((BR.AUTO, 2 * N - 5))
    assert lists[6][i - BE.ROW_N_LWE:i] == prods, "k = -1: the last step of the negative walk"
    g = lambda v: pow(5, v, 2 * N)
    # row 7: the sets at -20 and 20 are met with five steps pending (255 = 5 mod 10) and restart the count, so those at -10 and
    # 10 are met directly after the flush of a full window; row 8: the same one step beside; row 10: nine pending / a full window
    # flushed, in both walks
    pend = lambda row: [BE.pending_steps(N, lists[row], j) for j in range(4)]
    assert pend(7) == [g(10), g(5), g(10), g(5)]
    assert pend(8) == [g(3), g(4), g(2), g(2)]
    assert pend(10) == [g(9), g(10), g(10), g(9)] and lists[10][:2] == [(BR.AUTO, g(9)), (BR.PROD, 0)]


def test_schedule_edge_batches_and_the_fill(lib):
    """the selections of all rounds are 2 * rounds * B int32, two to a word, written 448 words per fill: one fill at B = 5, two at
    B = 7, three at B = 14"""
    logN, N = BE.ROW_LOGN, 1 << BE.ROW_LOGN
    rows = BE.rows()
    lens = [BR.rounds_of(BR.schedule(N, a)) for a in rows]
    ten = lib.Rounds(logN, rows[:10])
    assert len(ten) == max(lens[:10])
    for B in (5, 7, 14, len(rows)):
        idx = BE.batch_of(B) if B != len(rows) else list(range(B))
        rounds = lib.Rounds(logN, rows[idx])
        assert len(rounds) == max(lens[i] for i in idx)
        for b, i in enumerate(idx):
            got = []
            for gal, prod in rounds:
                if gal[b]:
                    got.append((BR.AUTO, int(gal[b])))
                if prod[b] >= 0:
                    got.append((BR.PROD, int(prod[b])))
            assert got == BR.schedule(N, rows[i]), (B, b)
        words = (2 * len(rounds) * B + 1) // 2
        assert {5: words <= BE.FILL_WORDS, 7: BE.FILL_WORDS < words <= 2 * BE.FILL_WORDS, 14: words > 2 * BE.FILL_WORDS}.get(B, True), (B, words)
    # some entries idle for many rounds while others work: rows 3 and 4 have nothing but automorphisms after / before their set
    idle = sum(1 for gal, prod in ten if prod[4] < 0 and any(prod[b] >= 0 for b in range(10)))
    assert idle >= 5


def test_blindrot_aliasing_rows_hold_against_the_header():
    import re
    from tests import blindrot_aliasing as BA
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hering_blindrot.h")).read(), flags=re.S)
    for name, row in BA.ROWS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m, name
        params = [p.split()[-1].lstrip("*") for p in m.group(1).split(",")]
        assert [p for p in params if p in row.params] == list(row.params), (name, params)
    sel, core = BA.ROWS["he_automorphism_ct_select"], BA.ROWS["he_blind_rotate_core"]
    assert sel.allowed == {("out0", "in0"), ("out1", "in1")}
    assert sel.verdict("in0", "in1") == "accept" and sel.verdict("out0", "out1") == "reject"
    assert sel.verdict("out0", "in1") == "reject" and sel.verdict("out1", "in0") == "reject"
    assert core.verdict("acc0", "acc1") == "reject" and not core.allowed
