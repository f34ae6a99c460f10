"""Ring-degree switching on the host (no GPU): the identity the device's one-pass fold rests on, checked on the oracle; the new
header's symbols, aliasing rows, Go and C++ mirrors.

The identity (core/rlwe/element.go:260-279): for a in [0, q)^N and both ring types,
    NTT_n(INTT_N(a)[::gap]) = gap^-1 * sum_{s<gap} a[j gap + s]  (mod q), canonical,
and the small ring's forward tables are a prefix of the large ring's (why the reference may run the large ring's tables at n)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from lattigo_amd import _lib
from oracle import oracle as O
from tests import ringswitch_aliasing as RS
from tests.helpers import rng_for, uniform_poly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hering_ringswitch.h")
NEW = ("he_map_small_to_large_ntt", "he_switch_ring_degree_ntt", "he_switch_ring_degree", "he_apply_evaluation_key")


def fold(a, q, gap):
    return np.array([(a[i].reshape(-1, gap).astype(object).sum(1) * pow(gap, -1, qi)) % qi for i, qi in enumerate(q)], dtype=np.uint64)


@pytest.mark.parametrize("ci", [False, True])
def test_fold_identity_and_table_prefix_on_the_oracle(ci):
    q, _ = O.GenModuli(16, [61, 50], [])  # = 1 mod 2^16: NTT-friendly for both ring types up to logN 14
    q = list(q)
    rng = rng_for(7000 + ci)
    for logN in range(5, 15):
        N = 1 << logN
        big = O.Ring(N, q, ci)
        a = uniform_poly(rng, q, N)
        top = np.array([[qi - 1] * N for qi in q], dtype=np.uint64)  # every word q - 1: the largest sums
        gap = 2
        while gap <= N // 16:
            small = O.Ring(N // gap, q, ci)
            for x in (a, top):
                ref = small.NTT(big.INTT(x)[:, ::gap].copy())
                assert np.array_equal(ref, fold(x, q, gap)), (logN, gap, ci)
            for i in range(len(q)):
                rs, rb = small.roots_forward(i), big.roots_forward(i)
                assert np.array_equal(rs, rb[: len(rs)]), (logN, gap, i)
            gap *= 2


def test_header_symbols_declared_and_exported():
    syms = _lib.declared_symbols()
    for s in NEW:
        assert s in syms, s
    so = _lib.lib_path()
    if not os.path.exists(so):
        pytest.skip("libhering.so not built")
    L = _lib.load()
    missing = [s for s in NEW if not hasattr(L, s)]
    assert not missing, missing
    # replayable: the recorder knows every new entry, with function ids after the last existing one
    ids = [_lib._TRACE_FNS[s][0] for s in NEW]
    assert sorted(ids) == list(range(51, 55)), ids


def test_aliasing_rows_are_the_header_entry_points():
    from tests.test_aliasing_table import poly_entries
    entries = poly_entries(open(HEADER).read())
    assert sorted(entries) == sorted(RS.ROWS), (sorted(entries), sorted(RS.ROWS))
    for name, params in entries.items():
        assert list(RS.ROWS[name].params) == params, (name, params)
    # the rule the header states: outputs never coincide; at equal degree every output may be any input
    ak = RS.ROWS["he_apply_evaluation_key"]
    assert ak.verdict("out0", "out1") == "reject"
    assert all(ak.verdict(o, i) == "accept" for o in ("out0", "out1") for i in ("in0", "in1"))
    for name in ("he_map_small_to_large_ntt", "he_switch_ring_degree_ntt", "he_switch_ring_degree"):
        o, i = list(RS.ROWS[name].params)[::-1]
        assert RS.ROWS[name].verdict(o, i) == "accept", name


def test_check_go_abi_reports_apply_evaluation_key():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_go_abi.py")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ApplyEvaluationKey" in out.stdout
    assert re.search(r"C\.he_apply_evaluation_key\(", open(os.path.join(ROOT, "go", "hering", "ringswitch.go")).read())


def test_cpp_mirror_compiles_with_the_new_methods(tmp_path):
    src = tmp_path / "rs.cpp"
    src.write_text("""#include "hering.hpp"
void f(const hering::Evaluator &ev, const hering::Ciphertext &a, const hering::EvaluationKey &k, hering::Ciphertext &b,
       const hering::Ring &r, const hering::Poly &ps, hering::Poly &pl) {
    ev.ApplyEvaluationKey(a, k, b);
    hering::SwitchCiphertextRingDegreeNTT(a, &r, b);
    hering::SwitchCiphertextRingDegreeNTT(a, nullptr, b);
    hering::SwitchCiphertextRingDegree(a, b);
    hering::MapSmallDimensionToLargerDimensionNTT(ps, pl);
}
""")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
