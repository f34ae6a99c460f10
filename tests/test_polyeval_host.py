"""include/hering_polyeval.h on the host (no device): OptimalSplit / SplitDegree / the depth check against the restatements of the
driver and the oracle; the library's structure of an evaluation (csrc/polyeval_plan.h through he_debug_polyeval_plan) against the
primitive calls oracle/polyeval_ref.evaluate_polynomial makes on the oracle backend -- the same (call, level, degree) sequence --
and the scales and scalar words lattigo_amd.polyeval plans against those the oracle-side evaluator computes in the same run."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import __graft_entry__ as graft
from drivers import polyeval as PE
from lattigo_amd import _lib
from oracle import circuits as OC
from oracle import oracle as O
from oracle import polyeval_ref as PR
from tests.helpers import rng_for
from tests.rlwe_fixtures import SecretKey, bgv_decrypt, bgv_encrypt, gen_evaluation_key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 9
T = 65537


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


@pytest.fixture(scope="module")
def pe(lib):
    from lattigo_amd import polyeval
    return polyeval


# ---- the integer helpers -------------------------------------------------------------------------------------------------------------
def test_optimal_split_split_degree_and_depth(lib, pe):
    for ld in range(1, 31):
        assert pe.OptimalSplit(ld) == PE.OptimalSplit(ld) == PR.optimal_split(ld), ld
    for n in list(range(1, 300)) + [1023, 1024, 1025, (1 << 20) + 3]:
        assert pe.SplitDegree(n) == PE.SplitDegree(n) == PR.split_degree(n), n
    for d in list(range(1, 70)) + [255, 256, 257]:
        assert pe.Depth(d) == ((d - 1).bit_length() if d > 1 else 0)
    assert lib.he_polyeval_split_degree(0, C.byref(C.c_int()), C.byref(C.c_int())) == -1
    assert b"invalid n: n=0 should be greater than zero" in lib.he_last_error()
    assert lib.he_polyeval_optimal_split(0, C.byref(C.c_int())) == -1
    assert pe.Depth(8, 3) == 3
    with pytest.raises(_lib.HeringError, match=r"2 levels < 3 log\(d\) -> cannot evaluate poly"):
        pe.Depth(8, 2)
    with pytest.raises(_lib.HeringError, match=r"3 levels < 4 log\(d\) -> cannot evaluate poly"):
        pe.Plan(9, level=3)
    with pytest.raises(_lib.HeringError, match=r"X\^\{1\} is nil"):
        pe.Plan(9, powers={2: (5, 1)})


# ---- the plan against the oracle's trace ----------------------------------------------------------------------------------------------
class RingSpy:
    """the oracle ring, recording the scalars of the constant and scalar-multiply calls an evaluation makes: one record per call
    of the evaluator (it repeats the ring call for every component of a ciphertext)"""

    def __init__(self, ring):
        self._r, self.words, self.ratios, self.fresh = ring, [], [], False

    def note(self, w, to=None):
        if self.fresh:
            (self.words if to is None else to).append(w)
        self.fresh = False

    def __getattr__(self, name):
        f = getattr(self._r, name)
        if name in ("AddScalarBigint", "MulScalarBigintThenAdd"):
            def call(x, v, *a):
                w = [int(v) % int(q) for q in self._r.moduli[: x.shape[0]]]
                self.note((w, w))
                return f(x, v, *a)
            return call
        if name in ("AddDoubleRNSScalar", "MulDoubleRNSScalarThenAdd", "MulDoubleRNSScalar"):
            def call(x, s0, s1, *a):
                self.note(([int(v) for v in s0], [int(v) for v in s1]), self.ratios if name == "MulDoubleRNSScalar" else None)
                return f(x, s0, s1, *a)
            return call
        return f


_RIGS = {}


def rig(kind):
    """logN 9, 8 + 2 limbs (top level 7), a relinearization key: the oracle backend of one scheme, built once"""
    if kind not in _RIGS:
        q, p = O.GenModuli(10, [55] + [45] * 7, [55, 55])
        rng = rng_for(7300 + len(kind))
        ringQ, ringP = O.Ring(N, q), O.Ring(N, p)
        ev = O.Evaluator(ringQ, ringP)
        sk = SecretKey(rng, ringQ, ringP)
        rlk = gen_evaluation_key(rng, ringQ, ringP, ringQ.binop("MulCoeffsMontgomery", sk.Q, sk.Q), sk)
        be = OC.BGVCtEvaluator(ev, T, rlk) if kind == "bgv" else OC.CKKSCtEvaluator(ev, rlk)
        _RIGS[kind] = (q, ringQ, sk, be)
    return _RIGS[kind]


def parity_mask(coeffs, parity):
    return [c if (parity == "both" or (k % 2 == 0) == (parity == "even")) else None for k, c in enumerate(coeffs)]


BGV_SHAPES = [(d, "Monomial", "both", False) for d in (1, 2, 3, 7, 8, 17, 33)] + [(12, "Monomial", "both", True)]
CKKS_SHAPES = [(1, "Monomial", "both", False), (7, "Monomial", "both", False), (12, "Monomial", "both", False),
               (5, "Chebyshev", "both", False), (31, "Chebyshev", "both", False), (30, "Chebyshev", "even", False),
               (31, "Chebyshev", "odd", False), (16, "Chebyshev", "even", False), (12, "Monomial", "both", True),
               (31, "Chebyshev", "both", True)]


def run_oracle(kind, deg, basis, parity, lazy, level=7):
    """(coefficients, input scale, target scale, the oracle's trace, the scalars it used, its result)"""
    q, ringQ, sk, be = rig(kind)
    rng = rng_for(7400 + 37 * deg + len(basis) + len(parity) + int(lazy))
    even, odd = parity in ("both", "even"), parity in ("both", "odd")
    sub = O.Ring(N, q[: level + 1])
    if kind == "bgv":
        coeffs = [int(x) for x in rng.integers(0, T, size=deg + 1)]
        coeffs[-1] = coeffs[-1] or 1
        scale, target = 3, 11
        ct = OC.Ct(list(bgv_encrypt(rng, sub, sk, rng.integers(0, T, size=N), T, scale)), scale)
    else:
        re, im = rng.uniform(-1, 1, size=deg + 1), rng.uniform(-1, 1, size=deg + 1)
        coeffs = [complex(a, b if basis == "Monomial" else 0.0) for a, b in zip(re, im)]
        scale = target = Fraction(1 << 45)
        ct = OC.Ct([np.stack([rng.integers(0, int(m), size=N, dtype=np.uint64) for m in q[: level + 1]]) for _ in range(2)], scale)
    masked = parity_mask(coeffs, parity)
    spy = RingSpy(be.ringQ)
    be.ringQ = spy

    def marked(f):
        def call(*a):
            spy.fresh = True
            try:
                return f(*a)
            finally:
                spy.fresh = False
        return call

    be.Add, be.MulThenAdd, be.Mul = marked(be.Add), marked(be.MulThenAdd), marked(be.Mul)
    try:
        tr = PR.Trace(be)
        res = PR.evaluate_polynomial(tr, ct, masked, target, basis, even, odd, lazy)
    finally:
        be.ringQ = spy._r
        del be.Add, be.MulThenAdd, be.Mul
    return masked, scale, target, tr.log, (spy.words, spy.ratios), res


@pytest.mark.parametrize("kind,deg,basis,parity,lazy", [("bgv",) + s for s in BGV_SHAPES] + [("ckks",) + s for s in CKKS_SHAPES])
def test_plan_scales_and_words_equal_the_oracle(pe, kind, deg, basis, parity, lazy):
    masked, scale, target, log, (words, ratios), res = run_oracle(kind, deg, basis, parity, lazy)
    q, ringQ, sk, be = rig(kind)
    even, odd = parity in ("both", "even"), parity in ("both", "odd")
    # the structure: the library's steps are the oracle's primitive calls
    plan = pe.Plan(deg, basis, even, odd, lazy, level=7)
    assert plan.log() == [(name, lvl, dg) for name, lvl, _, dg in log]
    assert plan.out_level == res.level == 7 - deg.bit_length()
    # the numbers: the mirror's scales after every step, and its scalar words in the order the oracle used them
    if kind == "bgv":
        scheme = pe.BGVScheme(q, T)
    else:
        scheme = pe.CKKSScheme(q, [O.MRed(int(ringQ.roots_forward(i)[1]), 1, int(m)) for i, m in enumerate(q)])
    planned = pe.Polynomial(masked, basis, even, odd, lazy).Plan(scheme, 7, scale, target)
    assert planned.scales == [s for _, _, s, _ in log]
    assert planned.out_scale == res.Scale == target
    mine = [(m[3], m[4]) for m in planned.minus_one] + [(w[1], w[2]) for f in planned.leaves for w in f["words"]]
    assert len(mine) == len(words)
    for i, (a, b) in enumerate(zip(mine, words)):
        assert (list(a[0]), list(a[1])) == b, i
    assert [(list(r[6]), list(r[7])) for r in planned.sub_ratio] == ratios  # the integer ratios of the Chebyshev Subs
    assert [(f["degree"], f["level"]) for f in planned.leaves] == [(f[0], f[1]) for f in plan.leaves]
    if any(f[0] == 0 for f in plan.leaves):
        print(f"{kind} {deg} {basis} {parity}: has a degree-0 baby step")


def test_an_even_chebyshev_polynomial_has_a_degree_zero_baby_step(pe):
    """the shape of the EvalMod polynomials: the reference allocates that baby step as a ciphertext of degree 0"""
    plan = pe.Plan(16, "Chebyshev", True, False, False, level=7)
    assert any(f[0] == 0 and f[2] == 0 and f[3] == 0 and f[4] == 1 for f in plan.leaves), plan.leaves


def test_evaluate_from_a_basis_that_holds_the_powers_generates_none(pe):
    first = pe.Plan(17, level=7)
    held = {1: (7, 1)}
    for op, dst, lvl, dg, a, b in first.steps:
        if dst > 0:
            held[dst] = (lvl, dg)
    again = pe.Plan(7, powers=held, copy_input=False)
    assert all(s[1] < 0 for s in again.steps)  # nothing but baby and giant steps
    more = pe.Plan(33, powers=held, copy_input=False)
    assert sorted({s[1] for s in more.steps if s[1] > 0}) == [32]  # made from the X^16 the basis holds, and rescaled


def test_the_oracle_result_decrypts_to_the_polynomial():
    """BGV degree 7 on the chain of these tests: the oracle's own result is p(m) mod t, so the GPU end-to-end test may rely on it"""
    q, ringQ, sk, be = rig("bgv")
    rng = rng_for(7777)
    m = rng.integers(0, T, size=N)
    coeffs = [int(x) for x in rng.integers(1, T, size=8)]
    ct = OC.Ct(list(bgv_encrypt(rng, ringQ, sk, m, T, 3)), 3)
    res = PR.evaluate_polynomial(be, ct, coeffs, 11)
    got = bgv_decrypt(O.Ring(N, q[: res.level + 1]), np.stack(res.Value), sk, T, res.Scale)
    from tests.rlwe_fixtures import negacyclic_mul_mod
    acc = np.zeros(N, dtype=np.int64)  # p(m) in Z_t[X]/(X^N + 1) by Horner
    for c in reversed(coeffs):
        acc = negacyclic_mul_mod(acc, m, T)
        acc[0] = (acc[0] + c) % T
    assert res.Scale == 11 and np.array_equal(got, acc)


def test_gen_power_plan_is_the_prefix_of_an_evaluation(lib, pe):
    """he_polyeval_gen_power_plan(2^k) lists the steps an evaluation's first GenPower makes"""
    whole = pe.Plan(17, level=7, copy_input=False)
    got = C.c_size_t()
    flat = (C.c_int * 3)(1, 7, 1)
    assert lib.he_polyeval_gen_power_plan(0, 16, 0, 1, flat, None, 0, C.byref(got)) == 0
    w = (C.c_int64 * got.value)()
    assert lib.he_polyeval_gen_power_plan(0, 16, 0, 1, flat, w, got.value, C.byref(got)) == 0
    steps = [tuple(int(x) for x in w[6 * i: 6 * i + 6]) for i in range(got.value // 6)]
    assert steps == whole.steps[: len(steps)] and steps[-1][:3] == (2, 16, 3)
    assert lib.he_polyeval_gen_power_plan(0, 0, 0, 1, flat, None, 0, C.byref(got)) == -1


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_a_wrong_leaf_list_is_einval(lib, pe):
    """number, degree and level of the caller's baby steps are held against the library's decomposition"""
    ints = lambda v: (C.c_int * max(len(v), 1))(*v)
    for deg, basis, parity, lazy in BGV_SHAPES + CKKS_SHAPES:
        even, odd = parity in ("both", "even"), parity in ("both", "odd")
        plan = pe.Plan(deg, basis, even, odd, lazy, level=7)
        degs, lvls = [f[0] for f in plan.leaves], [f[1] for f in plan.leaves]
        assert all(0 <= d <= pe.MAX_TERMS for d in degs) and all(0 <= x <= 7 for x in lvls)
        args = (deg, int(basis == "Chebyshev"), int(even), int(odd), int(lazy), 1, ints([1, 7, 1]))
        assert lib.he_polyeval_check_leaves(*args, len(degs), ints(degs), ints(lvls)) == 0, lib.he_last_error()
        assert lib.he_polyeval_check_leaves(*args, len(degs) + 1, ints(degs + [1]), ints(lvls + [1])) == -1
        assert b"baby steps given, the decomposition has" in lib.he_last_error()
        bad = list(degs)
        bad[-1] += 1
        assert lib.he_polyeval_check_leaves(*args, len(degs), ints(bad), ints(lvls)) == -1
        assert b"has degree" in lib.he_last_error()
        bad = list(lvls)
        bad[0] -= 1
        assert lib.he_polyeval_check_leaves(*args, len(degs), ints(degs), ints(bad)) == -1
        assert b"is at level" in lib.he_last_error()
    rc = lib.he_polyeval_poly_create(0, 7, 0, 1, 1, 0, 1, ints([1, 7, 1]), 1, ints([7]), ints([4]), None, None, C.byref(_lib.H()))
    assert rc == -2  # HE_EHANDLE: no ring


def test_the_scale_matching_of_a_chebyshev_sub(pe):
    """T_n = 2 T_a T_b - T_|a-b| subtracts a power at scale ~s from a product at scale ~s^2 that is not rescaled yet: the
    reference's evaluateInPlace multiplies the smaller operand by the truncated integer ratio (~s) first, in EVERY Chebyshev
    evaluation with a != b.  The mirror plans that ratio and its words (held against the oracle's in the shapes above); what it
    refuses is the BGV form, which would need matchScalesBinary."""
    sch = pe.CKKSScheme([1 << 45] * 3, [1, 1, 1])
    assert sch.sub_scale(Fraction(8), Fraction(8)) == (8, None, 1)
    assert sch.sub_scale(Fraction(9), Fraction(8)) == (9, 1, 1)
    assert sch.sub_scale(Fraction(16), Fraction(8)) == (16, 1, 2)
    assert sch.sub_scale(Fraction(5), Fraction(16)) == (16, 0, 3)
    assert pe.BGVScheme([97, 193], 17).sub_scale(3, 3) == (3, None, 1)
    with pytest.raises(ValueError, match="matchScalesBinary"):
        pe.BGVScheme([97, 193], 17).sub_scale(3, 5)


def test_the_ckks_branch_that_multiplies_the_accumulator_folds_into_the_earlier_words(pe):
    """MulThenAdd with op0.Scale == opOut.Scale and a constant that is no integer multiplies opOut by q_level first
    (schemes/ckks/evaluator.go:912-916): the same sum with every earlier word times q_level"""
    q, ringQ, sk, be = rig("ckks")
    sch = pe.CKKSScheme(q, [O.MRed(int(ringQ.roots_forward(i)[1]), 1, int(m)) for i, m in enumerate(q)])
    level, s = 2, Fraction(1 << 40)
    rng = rng_for(7900)
    X = OC.Ct([np.stack([rng.integers(0, int(m), size=N, dtype=np.uint64) for m in q[: level + 1]]) for _ in range(2)], s)
    out = be.NewCiphertext(1, level)
    out.Scale = s
    be.Add(out, (0.25, 0.5), out)
    be.MulThenAdd(X, (3, 0), out)        # an integer: the scales stay
    be.MulThenAdd(X, (0.3, -0.7), out)   # not an integer: out *= q_level
    words = [(0,) + tuple(list(w) for w in sch.const_words(level, s, sch.coeff((0.25, 0.5))))]
    scale = s
    for c in ((3, 0), (0.3, -0.7)):
        w, scale = sch.term(level, sch.coeff(c), s, scale, [x[1:] for x in words])
        words.append((1, list(w[0]), list(w[1])))
    assert scale == out.Scale == s * q[level]
    sub = O.Ring(N, q[: level + 1])
    half = N // 2
    want0 = np.zeros((level + 1, N), dtype=object)
    for i, m in enumerate(q[: level + 1]):
        for h, sl in ((1, slice(0, half)), (2, slice(half, N))):
            acc = np.full(sl.stop - sl.start, words[0][h][i], dtype=object)
            for w in words[1:]:
                acc = (acc + w[h][i] * X.Value[0][i][sl].astype(object)) % int(m)
            want0[i][sl] = acc
    assert np.array_equal(out.Value[0].astype(object), want0)
    del sub


# ---- the boundary's host side ----------------------------------------------------------------------------------------------------------
def test_header_symbols_and_recordings(lib):
    src = open(os.path.join(ROOT, "include", "hering_polyeval.h")).read()
    mine = sorted(set(re.findall(r"\b(he_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S))))
    assert mine == ["he_polyeval_basis_create", "he_polyeval_basis_destroy", "he_polyeval_basis_power", "he_polyeval_basis_powers",
                    "he_polyeval_check_leaves", "he_polyeval_depth", "he_polyeval_evaluate", "he_polyeval_evaluate_from_power_basis",
                    "he_polyeval_gen_power", "he_polyeval_gen_power_plan", "he_polyeval_leaves", "he_polyeval_optimal_split",
                    "he_polyeval_plan", "he_polyeval_poly_create", "he_polyeval_poly_destroy", "he_polyeval_poly_set_group",
                    "he_polyeval_split_degree"]
    assert all(s in _lib.declared_symbols() and hasattr(lib, s) for s in mine + ["he_debug_polyeval_plan"])
    tables = (_lib._TRACE_FNS, _lib._TRACE_FNS_RGSW, _lib._TRACE_FNS_BLINDROT, _lib._TRACE_FNS_BRIDGE, _lib._TRACE_FNS_BFV, _lib._TRACE_FNS_LINTRANS)
    for s in mine:
        assert not any(s in t for t in tables), s  # no replay numbers
        assert (s in _lib._TRACE_IGNORE) == (s not in ("he_polyeval_poly_create", "he_polyeval_leaves", "he_polyeval_basis_create",
                                                      "he_polyeval_gen_power", "he_polyeval_evaluate", "he_polyeval_evaluate_from_power_basis")), s
    names = [lib.he_prof_kernel_name(i).decode() for i in range(64)]
    assert names[names.index("diag_mac_group") + 1] == "poly_leaf_group"  # appended: earlier tests index the table
    hpp = open(os.path.join(ROOT, "include", "hering.hpp")).read()
    assert '#include "hering_polyeval.h"' in hpp and "hering_debug.h" not in hpp  # the mirrors read the plan through the boundary
    assert "he_debug_" not in open(os.path.join(ROOT, "lattigo_amd", "polyeval.py")).read()
    assert "he_debug_" not in open(os.path.join(ROOT, "go", "hering", "polyeval.go")).read()
    import lattigo_amd.polyeval as mod
    text = open(mod.__file__).read()
    assert "import tests" not in text and "from tests" not in text and "drivers" not in text
