"""BFV scale-invariant multiplication on the host (no GPU): the header's symbols, aliasing rows and mirrors, and the restatement of
the fused quantize kernel's per-coefficient arithmetic (tests/bfv_ref.py) against the coefficient-domain middle of the oracle's
`_quantize` -- BasisExtender.ModDownQPtoP, ModUpPtoQ, Ring.MulScalar (oracle/circuits.py:327-334) -- word for word.

Limb shapes (Q | QMul): (1 | 2), (3 x 36-bit | 2), (4 x 60-bit | 5), (3 | 3 of 61 bits) at logN 5 and 10, and four wider ones at
logN 5 up to the cap of 32 moduli on both sides; at every one the top level's levelQMul + 1 is the number of QMul moduli given.  Word sets: random, all zero, all q - 1 on both sides, and words chosen through the
reconstructions' own residues so that each float64 sum lands within one ulp of an integer: y_i = q_i - 1 on every limb (the sum
is n minus n roundings) and on a single limb (1 - 2^-53-ish, or exactly 1.0 for a 61-bit modulus whose (q - 1) / q rounds up)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from lattigo_amd import _lib
from oracle import circuits as OC
from oracle import oracle as O
from tests import bfv_aliasing as BA
from tests import bfv_ref as F
from tests.helpers import rng_for, uniform_poly
from tests.rlwe_fixtures import downstream_primes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hering_bfv.h")
NEW = ("he_bfv_evaluator_create", "he_bfv_evaluator_destroy", "he_bfv_level_qmul", "he_bfv_mul_relin", "he_bfv_quantize")
T = 65537

# (bits of the Q moduli, number of 61-bit QMul moduli)
SHAPES = {"1|2": ([58], 2), "3x36|2": ([36, 36, 36], 2), "4x60|5": ([60, 60, 60, 60], 5), "3|3x61": ([55, 55, 55], 3)}
# wider ones, one per instantiation of the kernel above four limbs of Q (8, 12, 16, 32), the last at the cap of both sides
WIDE = {"6x51|6": ([51] * 6, 6), "10x50|9": ([50] * 10, 9), "14x45|11": ([45] * 14, 11), "32x60|32": ([60] * 32, 32)}


def chain(logN, shape):
    """(Q moduli, QMul moduli) of a shape at ring degree 2^logN: NTT-friendly primes, QMul below 2^61 and disjoint from Q"""
    bits, nm = {**SHAPES, **WIDE}[shape]
    q, _ = O.GenModuli(logN + 1, bits, [])
    q = [int(x) for x in q]
    return q, downstream_primes(61, 2 << logN, nm, set(q))


def word_sets(rng, fz: F.Quantize, N):
    """{name: (cQ, cM)} coefficient-domain words, [nq, N] and [nm, N]"""
    Q, M = fz.Q, fz.M
    col = lambda ws, n: np.array([[w] * n for w in ws], dtype=np.uint64)
    sets = {"random": (uniform_poly(rng, Q, N), uniform_poly(rng, M, N)),
            "zero": (col([0] * len(Q), N), col([0] * len(M), N)),
            "top": (col([q - 1 for q in Q], N), col([m - 1 for m in M], N))}
    # float sums at an integer's edge: one coefficient per pattern, the rest random ("ulp", then "ulp1", ... when N is too small)
    pats = [([q - 1 for q in Q], [m - 1 for m in M])]                                    # every limb at the top: sums near n
    for i in range(len(Q)):                                                               # a single non-zero limb on the Q side
        pats.append(([q - 1 if k == i else 0 for k, q in enumerate(Q)], [0] * len(M)))
    for j in range(len(M)):                                                               # ... on the QMul side
        pats.append(([0] * len(Q), [m - 1 if k == j else 0 for k, m in enumerate(M)]))
    pats.append(([1] * len(Q), [1] * len(M)))                                             # sums of n tiny terms: v = 0
    for c in range(0, len(pats), N):
        cQ, cM = uniform_poly(rng, Q, N), uniform_poly(rng, M, N)
        for x, (yq, ym) in enumerate(pats[c: c + N]):
            a = fz.up.words_for_y(yq)
            cQ[:, x] = a
            cM[:, x] = fz.b_for_y2(a, ym)
            tr = {}
            fz.coefficient(a, cM[:, x], tr)
            assert tr["y"] == yq and tr["y2"] == ym, (x, tr)  # the construction reaches the residues it aims at
        sets["ulp" + (str(c // N) if c else "")] = (cQ, cM)
    return sets


def oracle_middle(be, ringQ, level, lm, cQ, cM, t):
    """oracle/circuits.py:331-333"""
    c2 = be.ModDownQPtoP(level, lm, cQ, cM)
    c1 = be.ModUpPtoQ(lm, level, c2)
    return ringQ.scalarop("MulScalar", c1, t)


@pytest.mark.parametrize("logN,shape", [(n, s) for n in (5, 10) for s in SHAPES] + [(5, s) for s in WIDE])
def test_fused_arithmetic_equals_the_oracles_quantize_middle(logN, shape):
    N = 1 << logN
    q, qm = chain(logN, shape)
    oQ, oM = O.Ring(N, q), O.Ring(N, qm)
    be = O.BasisExtender(oQ, oM)
    rng = rng_for(9100 + 10 * logN + list({**SHAPES, **WIDE}).index(shape))
    lq = F.level_qmul(q, logN)
    assert lq[-1] == len(qm) - 1, "the shape's top level uses every QMul modulus"
    levels = sorted({len(q) - 1, 0, max(len(q) - 2, 0)})
    for level in levels:
        lm = lq[level]
        fz = F.Quantize(q[: level + 1], qm[: lm + 1], T)
        for name, (cQ, cM) in word_sets(rng, fz, N).items():
            want = oracle_middle(be, O.Ring(N, q[: level + 1]), level, lm, cQ, cM, T)
            got = fz(cQ, cM)
            assert np.array_equal(got, want), (shape, level, name, np.argwhere(got != want)[:4])
            assert all((got[i] < np.uint64(q[i])).all() for i in range(level + 1)), "canonical"


def test_float_sums_reach_both_sides_of_an_integer():
    """the edge sets do what they are for.  With a modulus of 60 or 61 bits (q - 1) / q is 1.0 in float64 (q and q - 1 round to the
    same double), so a single top limb gives v = 1 where the exact quotient is below 1 and every limb at the top gives v = n, the
    last row of the table; with 36-bit moduli the quotient is exact enough: v = 0 and n - 1 (the truncation, not a rounding)."""
    for shape, single, full in (("4x60|5", 1, 4), ("3x36|2", 0, 2)):
        q, qm = chain(10, shape)
        fz, tr = F.Quantize(q, qm, T), {}
        top = [x - 1 for x in q]
        fz.coefficient(fz.up.words_for_y(top[:1] + [0] * (len(q) - 1)), [0] * len(qm), tr)
        assert tr["v"] == single, (shape, tr["v"])
        a = fz.up.words_for_y(top)
        fz.coefficient(a, fz.b_for_y2(a, [m - 1 for m in qm]), tr)
        assert tr["v"] == full and tr["v2"] == len(qm), (shape, tr["v"], tr["v2"])
        fz.coefficient(a, fz.b_for_y2(a, [qm[0] - 1] + [0] * (len(qm) - 1)), tr)
        assert tr["v2"] == 1, (shape, tr["v2"])


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("logN", [5, 10])
def test_level_qmul_equals_the_oracles_table(logN, shape):
    q, qm = chain(logN, shape)
    N = 1 << logN
    oQ, oM = O.Ring(N, q), O.Ring(N, qm)
    osi = OC.ScaleInvariantEvaluator(O.Evaluator(oQ, None), oM, T)
    assert F.level_qmul(q, logN) == osi.levelQMul


# ---- the header, the recorder and the mirrors ------------------------------------------------------------------------------------
def test_header_symbols_declared_and_exported():
    syms = _lib.declared_symbols()
    for s in NEW:
        assert s in syms, s
    assert os.path.exists(_lib.lib_path()), "libhering.so not built"
    L = _lib.load()
    missing = [s for s in NEW if not hasattr(L, s)]
    assert not missing, missing
    # replayable: the recorder knows the product entries, numbered on from the last existing one in a table of its own
    last = max(v[0] for t in (_lib._TRACE_FNS, _lib._TRACE_FNS_RGSW, _lib._TRACE_FNS_BLINDROT, _lib._TRACE_FNS_BRIDGE) for v in t.values())
    assert sorted(v[0] for v in _lib._TRACE_FNS_BFV.values()) == [last + 1, last + 2]
    assert set(_lib._TRACE_FNS_BFV) == {"he_bfv_mul_relin", "he_bfv_quantize"}
    names = [L.he_prof_kernel_name(i).decode() for i in range(64)]
    assert names.index("bfv_quantize") == names.index("ci_bridge_unfold") + 1


def test_header_states_its_domain():
    text = open(HEADER).read()
    for phrase in ("conjugate-invariant", "one by one", "ANY output may be\n * ANY input", "ring/basis_extension.go:285"):
        assert phrase in text, phrase


def test_aliasing_rows_are_the_header_entry_points():
    from tests.test_aliasing_table import poly_entries
    # (the evaluator handle `bfv` is no polynomial)
    entries = {n: [p for p in ps if p != "bfv"] for n, ps in poly_entries(open(HEADER).read()).items()}
    entries = {n: ps for n, ps in entries.items() if len(ps) >= 2}
    assert sorted(entries) == sorted(BA.ROWS)
    for name, params in entries.items():
        assert list(BA.ROWS[name].params) == params, (name, params)
    r = BA.ROWS["he_bfv_mul_relin"]
    outs, ins = ("out0", "out1", "out2"), ("a0", "a1", "b0", "b1")
    assert all(r.verdict(o, i) == "accept" for o in outs for i in ins)
    assert all(r.verdict(a, b) == "reject" for a in outs for b in outs if a != b)
    assert all(r.verdict(a, b) == "accept" for a in ins for b in ins if a != b)
    r = BA.ROWS["he_bfv_quantize"]
    assert r.verdict("outQ", "cQ") == "accept" and r.verdict("outQ", "cM") == "reject" and r.verdict("cQ", "cM") == "accept"


def test_check_go_abi_reports_the_bfv_file():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_go_abi.py")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bgv.Evaluator (scale-invariant): MulScaleInvariant, MulScaleInvariantNew, MulRelinScaleInvariant, MulRelinScaleInvariantNew" in out.stdout
    src = open(os.path.join(ROOT, "go", "hering", "bfv.go")).read()
    assert re.search(r"C\.he_bfv_mul_relin\(", src) and re.search(r"C\.he_bfv_evaluator_create\(", src)


def test_cpp_mirror_compiles_with_bfv():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "bfv_mirror.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
