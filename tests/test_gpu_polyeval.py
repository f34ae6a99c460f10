"""include/hering_polyeval.h on the device.  The baby steps of a polynomial evaluation through he_polyeval_leaves (the leaf-group
kernel), planned by lattigo_amd.polyeval: inside whole evaluations -- the power basis and the giant steps composed by
tests/drivers/polyeval.py from the operator entries -- word for word against oracle/polyeval_ref.py on the oracle backend and
against the unchanged driver; and alone, against the composed ring operations (he_double_rns_scalarop,
he_mul_scalar_bigint_then_add) on class-boundary chains with worst-case words."""
import ctypes as C
import math
import threading
from fractions import Fraction

import numpy as np
import pytest

import lattigo_amd as la
from drivers import polyeval as PE
from drivers.polyeval_native import NativeLeaves
from drivers import schemes as S
from lattigo_amd import _lib
from lattigo_amd import polyeval as NP
from oracle import circuits as OC
from oracle import oracle as O
from oracle import polyeval_ref as PR
from tests import boundary as Bd
from tests import polyeval_aliasing as A
from tests.gpu_common import ctx  # noqa: F401
from tests.helpers import rng_for
from tests.test_gpu_circuits import Rig

pytestmark = pytest.mark.gpu
GROUPS = (1, 2, 4)
T = 65537


# ---- whole evaluations: the driver with its baby steps handed to the library (tests/drivers/polyeval_native.py) ----------------------
def driver_poly(kind, masked, basis, parity, lazy):
    conv = (lambda c: c) if kind == "bgv" else PE._cpair
    pol = PE.Polynomial([None if c is None else conv(c) for c in masked], Basis=basis, Lazy=lazy)
    pol.IsEven, pol.IsOdd = parity in ("both", "even"), parity in ("both", "odd")
    return pol


def coeffs_for(kind, rng, deg, basis, parity):
    if kind == "bgv":
        c = [int(x) for x in rng.integers(0, T, size=deg + 1)]
        c[-1] = c[-1] or 1
    else:
        c = [complex(a, b if basis == "Monomial" else 0.0) for a, b in zip(rng.uniform(-1, 1, size=deg + 1), rng.uniform(-1, 1, size=deg + 1))]
    return [x if (parity == "both" or (k % 2 == 0) == (parity == "even")) else None for k, x in enumerate(c)]


def backends(rg, kind):
    if kind == "bgv":
        return S.BGVCiphertextEvaluator(rg.gev, T, rg.ggks.keys[1]), OC.BGVCtEvaluator(rg.oev, T, rg.ogks[1]), 3, 11
    scale = Fraction(1 << 45)
    return S.CKKSCiphertextEvaluator(rg.gev, rg.ggks.keys[1]), OC.CKKSCtEvaluator(rg.oev, rg.ogks[1]), scale, scale


def words_of(res):
    return np.stack([p.download() for p in res.Value], axis=1)  # [B][degree + 1][limbs][N]


SHAPES = [("bgv", d, "Monomial", "both", False) for d in (1, 2, 3, 7, 8, 17, 33)] + [
    ("ckks", 1, "Monomial", "both", False), ("ckks", 7, "Monomial", "both", False), ("ckks", 12, "Monomial", "both", False),
    ("ckks", 5, "Chebyshev", "both", False), ("ckks", 31, "Chebyshev", "both", False), ("ckks", 30, "Chebyshev", "even", False),
    ("ckks", 31, "Chebyshev", "odd", False), ("ckks", 16, "Chebyshev", "even", False), ("ckks", 12, "Monomial", "both", True),
    ("bgv", 12, "Monomial", "both", True)]


@pytest.mark.parametrize("kind,deg,basis,parity,lazy", SHAPES)
def test_whole_evaluation_against_the_oracle_and_the_driver(ctx, kind, deg, basis, parity, lazy):
    """the ring of test_bgv_polynomial_evaluation (logN 10, 8 + 2 limbs, top level 7), batch 2: the driver with native baby steps at
    G = 1, 2, 4 = the unchanged driver = the oracle's restatement, words, level, scale and degree; the input is untouched"""
    rg = Rig(ctx, 10, [55] + [45] * 7, [55, 55], 9100 + 31 * deg + len(basis) + len(parity) + int(lazy))
    rg.keys([1])
    gbe, obe, scale, target = backends(rg, kind)
    B, top = 2, 7
    ct = rg.ct(top, B)
    masked = coeffs_for(kind, rg.rng, deg, basis, parity)
    even, odd = parity in ("both", "even"), parity in ("both", "odd")
    gct = S.Ciphertext(rg.up(ct), top, scale)
    drv = PE.PolynomialEvaluator(gbe).Evaluate(gct, driver_poly(kind, masked, basis, parity, lazy), target)
    want_drv = words_of(drv)
    for G in GROUPS:
        ne = NativeLeaves(gbe, rg.pr.gQ, G)
        res = ne.Evaluate(gct, driver_poly(kind, masked, basis, parity, lazy), target)
        assert ne.calls == 1
        assert (res.Scale, res.level, res.Degree()) == (drv.Scale, drv.level, drv.Degree()) == (target, top - deg.bit_length(), 1)
        assert (ne.planned.out_scale, ne.planned.out_level) == (res.Scale, res.level)
        assert np.array_equal(words_of(res), want_drv), G
    for b in range(B):
        want = PR.evaluate_polynomial(obe, OC.Ct(list(ct[b]), scale), masked, target, basis, even, odd, lazy)
        assert (drv.Scale, drv.level, drv.Degree()) == (want.Scale, want.level, want.Degree())
        assert np.array_equal(want_drv[b][:, : drv.level + 1], np.stack(want.Value)), b
    assert np.array_equal(gct.Value[0].download(), ct[:, 0]) and np.array_equal(gct.Value[1].download(), ct[:, 1])


@pytest.mark.parametrize("B", [1, 3, 5])
def test_batches_that_do_not_fill_a_tile(ctx, B):
    rg = Rig(ctx, 10, [55] + [45] * 7, [55, 55], 9200 + B)
    rg.keys([1])
    for kind, deg, basis, lazy in (("bgv", 7, "Monomial", False), ("ckks", 12, "Monomial", True), ("ckks", 16, "Chebyshev", False)):
        gbe, obe, scale, target = backends(rg, kind)
        ct = rg.ct(7, B)
        masked = coeffs_for(kind, rg.rng, deg, basis, "both")
        gct = S.Ciphertext(rg.up(ct), 7, scale)
        want = words_of(PE.PolynomialEvaluator(gbe).Evaluate(gct, driver_poly(kind, masked, basis, "both", lazy), target))
        for G in GROUPS:
            res = NativeLeaves(gbe, rg.pr.gQ, G).Evaluate(gct, driver_poly(kind, masked, basis, "both", lazy), target)
            assert np.array_equal(words_of(res), want), (kind, G)
        ref = PR.evaluate_polynomial(obe, OC.Ct(list(ct[B - 1]), scale), masked, target, basis, True, True, lazy)
        assert np.array_equal(want[B - 1][:, : ref.level + 1], np.stack(ref.Value)), kind


def _prof(ctx, call):
    call()
    ctx.sync()
    ctx.prof_begin()
    call()
    ctx.sync()
    return {k: v[0] for k, v in ctx.prof_end().items() if v[0]}


def test_two_polynomials_on_one_basis_and_the_launch_census(ctx):
    """EvaluateFromPowerBasis: the second polynomial finds every power it needs -- its plan has no power step -- and its baby steps
    are ceil(n / G) launches of the leaf-group kernel and nothing else, where the composed path makes one element-wise launch per
    constant and per (term, component)"""
    rg = Rig(ctx, 10, [55] + [45] * 7, [55, 55], 9300)
    rg.keys([1])
    gbe, obe, scale, target = backends(rg, "bgv")
    B, top = 2, 7
    gct = S.Ciphertext(rg.up(rg.ct(top, B)), top, scale)
    first = coeffs_for("bgv", rg.rng, 17, "Monomial", "both")
    second = coeffs_for("bgv", rg.rng, 15, "Monomial", "both")
    # the basis of the first evaluation, kept
    drv = PE.PolynomialEvaluator(gbe)
    pb = PE.PowerBasis(gct, gbe)
    pb.GenPower(16, False, gbe)
    for i in range((1 << PE.OptimalSplit(5)) - 1, 2, -1):
        pb.GenPower(i, False, gbe)
    PS = PE.PatersonStockmeyerPolynomial(driver_poly("bgv", first, "Monomial", "both", False), top, scale, target, drv.sim)
    want_first = words_of(drv.EvaluatePatersonStockmeyerPolynomial(PS, pb))
    held = {n: (x.level, x.Degree(), x.Scale) for n, x in pb.Value.items()}
    assert sorted(held) == [1, 2, 3, 4, 5, 6, 7, 8, 16]
    ne = NativeLeaves(gbe, rg.pr.gQ)
    pl = ne.plan(driver_poly("bgv", first, "Monomial", "both", False), top, scale, target, powers=held)
    assert all(s[1] < 0 for s in pl.plan.steps)
    PS = PE.PatersonStockmeyerPolynomial(driver_poly("bgv", first, "Monomial", "both", False), top, scale, target, drv.sim)
    assert np.array_equal(words_of(ne.EvaluatePatersonStockmeyerPolynomial(PS, pb)), want_first)
    # the second polynomial (degree 15: X^2, X^3 for its baby steps, X^4 and X^8 for its giant steps) on the same basis
    pol2 = lambda: driver_poly("bgv", second, "Monomial", "both", False)
    PS2 = lambda: PE.PatersonStockmeyerPolynomial(pol2(), top, scale, target, drv.sim)
    want = words_of(drv.EvaluatePatersonStockmeyerPolynomial(PS2(), pb))
    for G in GROUPS:
        ne = NativeLeaves(gbe, rg.pr.gQ, G)
        pl = ne.plan(pol2(), top, scale, target, powers=held)
        assert all(s[1] < 0 for s in pl.plan.steps) and len(pb.Value) == 9  # no power is made
        assert np.array_equal(words_of(ne.EvaluatePatersonStockmeyerPolynomial(PS2(), pb)), want), G
        # census of the baby steps alone
        outs = [[la.Poly(rg.pr.gQ, f["level"] + 1, B) for _ in range(f["ct_degree"] + 1)] for f in pl.leaves]
        X = {k: x.Value for k, x in pb.Value.items()}
        got = _prof(ctx, lambda: pl.EvaluatePolynomialFromPowerBasis(X, outs))
        assert got == {"poly_leaf_group": math.ceil(len(pl.leaves) / G)}, (G, got)
    # the composed path, from separately profiled pieces: per baby step its two new (zero-filled) polynomials, one launch for the
    # constant and one per (term, component)
    scratch = [la.Poly(rg.pr.gQ, 4, B), la.Poly(rg.pr.gQ, 4, B)]
    one_term = _prof(ctx, lambda: rg.pr.gQ.AtLevel(3).MulScalarBigintThenAdd(scratch[0], 5, scratch[1]))
    one_const = _prof(ctx, lambda: rg.pr.gQ.AtLevel(3).AddScalarBigint(scratch[0], 5, scratch[0]))
    one_new = _prof(ctx, lambda: la.Poly(rg.pr.gQ, 4, B))
    assert one_term == {"ew": 1} and one_const == {"ew": 1}
    composed = _prof(ctx, lambda: [drv.EvaluateBabyStep(p, pb) for p in PS2()])
    terms = sum(bin(f[4] >> 1).count("1") for f in pl.plan.leaves)
    consts = sum(f[4] & 1 for f in pl.plan.leaves)
    want = {}
    for piece, times in ((one_term, 2 * terms), (one_const, consts), (one_new, 2 * len(pl.plan.leaves))):
        for k, c in piece.items():
            want[k] = want.get(k, 0) + times * c
    print("composed baby steps:", composed, "native:", got)
    assert composed == want, (composed, want)
    assert sum(composed.values()) >= 2 * terms + consts > sum(got.values())


# ---- lattigo_amd.polyeval.Evaluator: the library's plan run over the operator entries -----------------------------------------------------
def mirror(rg, kind):
    gbe, obe, scale, target = backends(rg, kind)
    scheme = NP.BGVScheme(rg.q, T) if kind == "bgv" else NP.CKKSScheme.for_ring(rg.pr.gQ)
    return NP.Evaluator(rg.gev, scheme, rg.ggks.keys[1]), gbe, obe, scale, target


@pytest.mark.parametrize("kind,deg,basis,parity,lazy", SHAPES)
def test_mirror_evaluator_against_the_driver_and_the_oracle(ctx, kind, deg, basis, parity, lazy):
    """Evaluator.Evaluate of the shipped mirror -- every step in the order of he_debug_polyeval_plan, the baby steps in one
    he_polyeval_leaves call -- equals the driver and the oracle: words, level, scale, degree; G = 1, 2, 4; the input untouched"""
    rg = Rig(ctx, 10, [55] + [45] * 7, [55, 55], 9900 + 31 * deg + len(basis) + len(parity) + int(lazy))
    rg.keys([1])
    me, gbe, obe, scale, target = mirror(rg, kind)
    B, top = 2, 7
    ct = rg.ct(top, B)
    masked = coeffs_for(kind, rg.rng, deg, basis, parity)
    even, odd = parity in ("both", "even"), parity in ("both", "odd")
    drv = PE.PolynomialEvaluator(gbe).Evaluate(S.Ciphertext(rg.up(ct), top, scale), driver_poly(kind, masked, basis, parity, lazy), target)
    want = words_of(drv)
    gct = NP.Ciphertext(rg.up(ct), top, scale)
    pol = NP.Polynomial(masked, basis, even, odd, lazy)
    for G in (0,) + GROUPS:
        me.SetGroup(G)
        res = me.Evaluate(gct, pol, target)
        assert (res.Scale, res.level, res.Degree()) == (drv.Scale, drv.level, drv.Degree()) == (target, top - deg.bit_length(), 1), G
        assert np.array_equal(words_of(res)[:, :, : res.level + 1], want[:, :, : drv.level + 1]), G
    ref = PR.evaluate_polynomial(obe, OC.Ct(list(ct[1]), scale), masked, target, basis, even, odd, lazy)
    assert np.array_equal(words_of(res)[1][:, : res.level + 1], np.stack(ref.Value))
    assert np.array_equal(gct.Value[0].download(), ct[:, 0]) and np.array_equal(gct.Value[1].download(), ct[:, 1])


@pytest.mark.parametrize("kind,basis", [("bgv", "Monomial"), ("ckks", "Chebyshev")])
def test_native_evaluate_from_power_basis_census_and_refusals(ctx, kind, basis):
    """he_polyeval_evaluate_from_power_basis: three polynomials on one basis.  The second finds every power it needs: the basis is
    unchanged and the call's launches are the giant steps' -- kernel for kernel the driver's on the same basis -- plus ceil(n / G)
    leaf-group launches, with fewer element-wise launches than the driver; the third makes X^32 from the X^16 it finds.  A
    refused call changes neither an operand nor the basis."""
    rg = Rig(ctx, 10, [55] + [45] * 7, [55, 55], 9950 + len(kind))
    rg.keys([1])
    me, gbe, obe, scale, target = mirror(rg, kind)
    B, top = 3, 7
    ct = rg.ct(top, B)
    gct = NP.Ciphertext(rg.up(ct), top, scale)
    pb = me.NewPowerBasis(gct, basis)
    drv = PE.PolynomialEvaluator(gbe)
    dct = S.Ciphertext(rg.up(ct), top, scale)
    for n, deg in enumerate((17, 15, 33)):
        masked = coeffs_for(kind, rg.rng, deg, basis, "both")
        before = pb.Powers()
        res = me.EvaluateFromPowerBasis(pb, NP.Polynomial(masked, basis), target)
        assert (pb.Powers() == before) == (n == 1), (n, pb.Powers())
        want = drv.Evaluate(dct, driver_poly(kind, masked, basis, "both", False), target)
        assert (res.Scale, res.level) == (want.Scale, want.level)
        assert np.array_equal(words_of(res)[:, :, : res.level + 1], words_of(want)[:, :, : want.level + 1]), deg
        if n == 1:  # the census of a call that generates no power
            pol = NP.Polynomial(masked, basis)
            dpb = PE.PowerBasis(dct, gbe, basis)
            dpb.GenPower(16, False, gbe)
            for i in range(7, 2, -1):
                dpb.GenPower(i, False, gbe)
            assert all(np.array_equal(pb.Words(k)[:, :, : x.level + 1], words_of(x)[:, :, : x.level + 1]) for k, x in dpb.Value.items())
            PS = lambda: PE.PatersonStockmeyerPolynomial(driver_poly(kind, masked, basis, "both", False), top, scale, target, drv.sim)
            composed = _prof(ctx, lambda: drv.EvaluatePatersonStockmeyerPolynomial(PS(), dpb))
            for G in GROUPS:
                me.SetGroup(G)
                got = _prof(ctx, lambda: me.EvaluateFromPowerBasis(pb, pol, target))
                leaves = len(me._planned(pb.held(), pol, target).leaves)
                assert got.pop("poly_leaf_group") == math.ceil(leaves / G), (G, got)
                assert {k: v for k, v in got.items() if k != "ew"} == {k: v for k, v in composed.items() if k != "ew"}, (G, got, composed)
                assert got.get("ew", 0) < composed["ew"], (got, composed)
            me.SetGroup(0)
            assert pb.Powers() == before
    assert np.array_equal(gct.Value[0].download(), ct[:, 0])
    # GenPower as a call of its own: the words of the driver's
    pb2, dpb = me.NewPowerBasis(gct, basis), PE.PowerBasis(dct, gbe, basis)
    for n, lazy in ((4, False), (7, True), (6, False)):
        me.GenPower(pb2, n, lazy)
        dpb.GenPower(n, lazy, gbe)
        assert pb2.Powers() == {k: (x.level, x.Degree()) for k, x in dpb.Value.items()}, n
        assert all(pb2.Scale[k] == x.Scale for k, x in dpb.Value.items())
        assert all(np.array_equal(pb2.Words(k)[:, :, : x.level + 1], words_of(x)[:, :, : x.level + 1]) for k, x in dpb.Value.items()), n
    # refusals, each before anything is filed
    snap = lambda: [pb.Words(k).copy() for k in sorted(pb.Powers())] + [gct.Value[0].download(), gct.Value[1].download()]
    state, powers = snap(), pb.Powers()

    def rejected(call, match):
        with pytest.raises(_lib.HeringError, match=match) as e:
            call()
        assert e.value.code == -1
        ctx.sync()
        assert pb.Powers() == powers and all(np.array_equal(a, b) for a, b in zip(snap(), state))

    low = NP.Ciphertext(rg.up(rg.ct(2, 1)), 2, scale)
    rejected(lambda: me.Evaluate(low, NP.Polynomial(coeffs_for(kind, rg.rng, 7, basis, "both"), basis), target), r"2 levels < 3 log\(d\) -> cannot evaluate poly")
    nokey = NP.Evaluator(rg.gev, me.scheme, None)
    p65 = NP.Polynomial(coeffs_for(kind, rg.rng, 65, basis, "both"), basis)  # needs X^64: a relinearization
    rejected(lambda: nokey.EvaluateFromPowerBasis(pb, p65, target), "RelinearizationKey is nil")
    rejected(lambda: nokey.Evaluate(gct, NP.Polynomial(coeffs_for(kind, rg.rng, 3, basis, "both"), basis), target), "RelinearizationKey is nil")
    # operand identity at the two evaluation entries (tests/polyeval_aliasing.py): no output may be an input, a power, or the other output
    assert all(r.allowed == set() for r in A.ROWS.values())
    pol3 = NP.Polynomial(coeffs_for(kind, rg.rng, 3, basis, "both"), basis)
    pl = me._planned({1: (top, 1, scale)}, pol3, target)
    n_aux, kinds, s0, s1, L = NP._aux(pl)
    L_ = _lib.load()
    outs = [la.Poly(rg.pr.gQ, top + 1, B), la.Poly(rg.pr.gQ, top + 1, B)]
    args = lambda o0, o1: (rg.gev.h, pl.h, *me._scheme_args(), top, gct.Value[0].h, gct.Value[1].h, n_aux, kinds, s0.ctypes.data_as(_lib.u64p),
                           s1.ctypes.data_as(_lib.u64p), L, o0.h, o1.h)
    for o0, o1 in ((gct.Value[0], outs[1]), (outs[0], gct.Value[1]), (gct.Value[1], gct.Value[0]), (outs[0], outs[0])):
        rejected(lambda: _lib.check(L_.he_polyeval_evaluate(*args(o0, o1))), "an output is a component of the input|the same polynomial")
    small = la.Poly(rg.pr.gQ, 1, B)
    rejected(lambda: _lib.check(L_.he_polyeval_evaluate(*args(small, outs[1]))), "too few limbs")
    _lib.check(L_.he_polyeval_evaluate(*args(*outs)))  # and the same call with proper outputs runs
    pl = me._planned(pb.held(), pol3, target)
    n_aux, kinds, s0, s1, L = NP._aux(pl)
    fargs = lambda o0, o1: (pb.h, pl.h, *me._scheme_args(), n_aux, kinds, s0.ctypes.data_as(_lib.u64p), s1.ctypes.data_as(_lib.u64p), L, o0.h, o1.h)
    comps = (_lib.H * 3)()
    _lib.check(L_.he_polyeval_basis_power(pb.h, 2, comps))

    class Borrowed:
        h = comps[0]
    rejected(lambda: _lib.check(L_.he_polyeval_evaluate_from_power_basis(*fargs(Borrowed, outs[1]))), "an output is a component of X")
    rejected(lambda: _lib.check(L_.he_polyeval_evaluate_from_power_basis(*fargs(outs[1], outs[1]))), "the same polynomial")
    other = me.NewPowerBasis(gct, basis)  # a basis of another shape than the polynomial was planned for
    rejected(lambda: _lib.check(L_.he_polyeval_evaluate_from_power_basis(other.h, *fargs(*outs)[1:])), "planned for")
    rejected(lambda: _lib.check(L_.he_polyeval_evaluate_from_power_basis(*fargs(*outs)[:5], n_aux + 1, *fargs(*outs)[6:])), "Chebyshev")
    assert np.array_equal(gct.Value[0].download(), ct[:, 0]) and np.array_equal(gct.Value[1].download(), ct[:, 1])


@pytest.mark.parametrize("deferred", [0, 4])
def test_native_evaluate_queue_coalesced_and_deferred(ctx, deferred):
    """4 threads, each evaluating its own batch-1 ciphertext through he_polyeval_evaluate: bit-identical to the direct calls"""
    rg = Rig(ctx, 10, [55] + [45] * 7, [55, 55], 9970 + deferred)
    rg.keys([1])
    me, gbe, obe, scale, target = mirror(rg, "ckks")
    pol = NP.Polynomial(coeffs_for("ckks", rg.rng, 12, "Chebyshev", "both"), "Chebyshev")
    TH = 4
    cts = [NP.Ciphertext(rg.up(rg.ct(7, 1)), 7, scale) for _ in range(TH)]
    want = [words_of(me.Evaluate(c, pol, target)) for c in cts]
    ctx.sync()
    got = [None] * TH
    ctx.SetCoalescing(64, 2000)
    if deferred:
        ctx.SetDeferred(deferred)
    try:
        barrier, errs = threading.Barrier(TH), []

        def worker(t):
            try:
                barrier.wait()
                for _ in range(2):
                    got[t] = me.Evaluate(cts[t], pol, target)
            except Exception as e:  # noqa: BLE001
                errs.append(e)
                barrier.abort()

        th = [threading.Thread(target=worker, args=(t,)) for t in range(TH)]
        [x.start() for x in th]
        [x.join() for x in th]
        ctx.sync()
        assert not errs, errs
    finally:
        if deferred:
            ctx.SetDeferred(0)
        ctx.SetCoalescing(0, 0)
    for t in range(TH):
        assert np.array_equal(words_of(got[t]), want[t]), t


# ---- the leaf entry alone, against the composed ring operations --------------------------------------------------------------------------
def make_handle(ring, degree, basis, even, odd, lazy, powers, plan, s0, s1):
    ints = lambda v: (C.c_int * max(len(v), 1))(*[int(x) for x in v])
    flat = [v for n in sorted(powers) for v in (n,) + tuple(powers[n])]
    h = _lib.H()
    _lib.check(_lib.load().he_polyeval_poly_create(ring.h, degree, int(basis == "Chebyshev"), int(even), int(odd), int(lazy), len(powers),
                                                 ints(flat), len(plan.leaves), ints([f[0] for f in plan.leaves]), ints([f[1] for f in plan.leaves]),
                                                 s0.ctypes.data_as(_lib.u64p), s1.ctypes.data_as(_lib.u64p), C.byref(h)))
    return h.value


class LeafCase:
    """a polynomial shape on a chain, scalar words and powers of chosen kinds: the library's baby steps against the reference's
    sequence -- Add(res, c_0), then MulThenAdd(X[k], c_k, res) for k = deg ... 1, the accumulator resized to the degree of each
    X[k] in turn -- made of ring operations on the device"""

    def __init__(self, ctx, logN, letters, degree, B, seed, basis="Monomial", parity="both", xdeg=None, kinds=Bd.WORST_CASE_KINDS,
                 scalars="uniform", bigint=False):
        self.q = Bd.class_chain(logN, letters)
        self.N, self.B, self.level = 1 << logN, B, len(self.q) - 1
        self.ring = la.Ring(ctx, self.N, self.q)
        rng = self.rng = rng_for(seed)
        self.even, self.odd = parity in ("both", "even"), parity in ("both", "odd")
        shape = NP.Plan(degree, basis, self.even, self.odd, False, level=self.level)
        need = max([f[0] for f in shape.leaves] + [1])
        self.xdeg = {k: (xdeg or {}).get(k, 1) for k in range(1, need + 1)}
        self.powers = {k: (self.level, d) for k, d in self.xdeg.items()}
        self.plan = NP.Plan(degree, basis, self.even, self.odd, False, powers=self.powers, copy_input=False)
        assert [f[:2] for f in self.plan.leaves] == [f[:2] for f in shape.leaves]
        L = self.level + 1
        rows = sum(f[0] + 1 for f in self.plan.leaves)
        if scalars == "max":
            s0 = np.array([[m - 1 for m in self.q]] * rows, dtype=np.uint64)
            s1 = s0.copy()
        else:
            s0 = np.stack([rng.integers(0, int(m), size=rows, dtype=np.uint64) for m in self.q], axis=1)
            s1 = s0.copy() if bigint else np.stack([rng.integers(0, int(m), size=rows, dtype=np.uint64) for m in self.q], axis=1)
        self.bigint = bigint
        if bigint:  # one integer per scalar, as BGV has them: its residues are the words
            self.big = [int(rng.integers(0, 1 << 62)) * int(rng.integers(1, 1 << 62)) for _ in range(rows)]
            s0 = np.array([[v % m for m in self.q] for v in self.big], dtype=np.uint64)
            s1 = s0.copy()
        self.s0, self.s1 = np.ascontiguousarray(s0), np.ascontiguousarray(s1)
        assert self.s0.shape == (rows, L)
        self.h = make_handle(self.ring, degree, basis, self.even, self.odd, False, self.powers, self.plan, self.s0, self.s1)
        cyc = Bd.WordCycle(kinds, seed)
        self.X = {k: [la.Poly(self.ring, L, B).upload(np.stack([cyc(rng, self.q, self.N) for _ in range(B)])) for _ in range(d + 1)]
                  for k, d in self.xdeg.items()}

    def close(self):
        _lib.load().he_polyeval_poly_destroy(self.h)

    def outs(self, first=0, count=None):
        leaves = self.plan.leaves[first: None if count is None else first + count]
        return [[la.Poly(self.ring, f[1] + 1, self.B, zero=False) for _ in range(f[3] + 1)] for f in leaves]

    def run(self, G, first=0, count=None, outs=None):
        _lib.check(_lib.load().he_polyeval_poly_set_group(self.h, G))
        count = len(self.plan.leaves) - first if count is None else count
        outs = self.outs(first, count) if outs is None else outs
        top = max([f[0] for f in self.plan.leaves[first: first + count]] + [0])
        xs = (_lib.H * max(3 * top, 1))()
        for k in range(1, top + 1):
            for c, p in enumerate(self.X[k]):
                xs[3 * (k - 1) + c] = p.h
        os_ = (_lib.H * (3 * count))()
        for g in range(count):
            for c, p in enumerate(outs[g]):
                os_[3 * g + c] = p.h
        _lib.check(_lib.load().he_polyeval_leaves(self.h, first, count, top, xs, os_))
        return outs

    def composed(self):
        """[leaf] -> [B][components][level + 1][N]"""
        out, row = [], 0
        for deg, lvl, newdeg, ctdeg, present in self.plan.leaves:
            r = self.ring.AtLevel(lvl)
            res = [la.Poly(self.ring, lvl + 1, self.B) for _ in range(newdeg + 1)]
            if present & 1:
                if self.bigint:
                    r.AddScalarBigint(res[0], self.big[row], res[0])
                else:
                    r.AddDoubleRNSScalar(res[0], self.s0[row][: lvl + 1], self.s1[row][: lvl + 1], res[0])
            for k in range(deg, 0, -1):
                if not (present >> k) & 1:
                    continue
                x = self.X[k]
                res = res[: len(x)] + [la.Poly(self.ring, lvl + 1, self.B) for _ in range(len(x) - len(res))]  # Resize(op0.Degree())
                for c in range(len(x)):
                    if self.bigint:
                        r.MulScalarBigintThenAdd(x[c], self.big[row + k], res[c])
                    else:
                        r.MulDoubleRNSScalarThenAdd(x[c], self.s0[row + k][: lvl + 1], self.s1[row + k][: lvl + 1], res[c])
            assert len(res) == ctdeg + 1
            out.append(np.stack([p.download() for p in res], axis=1))
            row += deg + 1
        return out

    def check(self, groups=GROUPS):
        want = self.composed()
        for G in groups:
            got = self.run(G)
            for i, (o, w) in enumerate(zip(got, want)):
                assert np.array_equal(np.stack([p.download() for p in o], axis=1), w), (G, i)
        return want


CHAIN11 = "hiIdDhidhid"  # eleven limbs across the 47- / 58- / 61-bit classes: level 10, the depth of a polynomial of degree 1023


def test_leaf_chains_are_what_they_claim():
    for logN, letters in ((4, CHAIN11), (8, "hiIdD"), (9, "dhiDIh"), (8, "h" * 11)):
        q = Bd.class_chain(logN, letters)
        assert len(set(q)) == len(letters) and all(m % (2 << logN) == 1 for m in q)


def test_leaf_half_boundary_inside_one_wave_and_the_largest_leaves(ctx):
    """logN 4: both halves of a limb -- the two residues of a scalar -- inside one wave; degree 1023: 37 baby steps at levels 1 .. 10,
    31 of them of 31 terms, the most the entry admits; batch 3 leaves the tile of two entries half empty"""
    case = LeafCase(ctx, 4, CHAIN11, 1023, 3, 9400)
    degs = [f[0] for f in case.plan.leaves]
    assert len(degs) == 37 and max(degs) == NP.MAX_TERMS and degs.count(NP.MAX_TERMS) == 31
    assert all(len({f[1] for f in case.plan.leaves[i: i + 4]}) > 1 for i in range(0, 36, 4))  # every group of four spans levels
    case.check()
    case.close()


def test_leaf_every_word_and_scalar_at_its_maximum(ctx):
    """eleven 61-bit primes, every word of every power, every scalar and every constant q - 1, 31 terms: the accumulation is exact"""
    case = LeafCase(ctx, 8, "h" * 11, 1023, 1, 9410, kinds=("max",), scalars="max")
    want = case.check()
    # a baby step of d terms: (q - 1) + d (q - 1)^2 = d - 1 mod q on component 0, d on component 1
    for f, w in zip(case.plan.leaves, want):
        assert all(int(w[0][0][l][j]) == f[0] - 1 and int(w[0][1][l][j]) == f[0] for l in range(w.shape[2]) for j in (0, case.N - 1)), f
    case.close()


@pytest.mark.parametrize("logN,letters,degree,B,parity,basis", [(8, "hiIdD", 12, 5, "both", "Monomial"), (9, "dhiDIh", 17, 2, "odd", "Monomial"),
                                                                 (9, "dhiDIh", 16, 2, "even", "Chebyshev"), (4, "hiIdD", 7, 4, "both", "Monomial")])
def test_leaf_shapes_across_the_classes(ctx, logN, letters, degree, B, parity, basis):
    case = LeafCase(ctx, logN, letters, degree, B, 9420 + logN + degree, basis=basis, parity=parity)
    if parity == "even" and degree == 16:
        assert any(f[0] == 0 and f[3] == 0 for f in case.plan.leaves)  # the degree-0 baby step: a result of ONE polynomial
    case.check()
    case.close()


@pytest.mark.parametrize("xdeg", [{3: 2}, {1: 2, 2: 2, 3: 2}, {1: 2, 3: 2}, {2: 2}], ids=["x3", "all", "x1-x3", "x2"])
def test_leaf_powers_of_degree_two(ctx, xdeg):
    """lazy powers: the reference's accumulator takes the degree of each power in turn, so the third component of a power
    survives only where every lower power has one, and the result has the degree of X^1"""
    case = LeafCase(ctx, 8, "hiIdD", 12, 3, 9430 + sum(xdeg), xdeg=xdeg)
    assert all(f[3] == xdeg.get(1, 1) for f in case.plan.leaves if f[4] >> 1)
    case.check()
    case.close()


def test_leaf_against_the_bigint_form(ctx):
    """BGV: one integer per scalar through he_add_scalar_bigint / he_mul_scalar_bigint_then_add"""
    case = LeafCase(ctx, 8, "hiIdD", 12, 2, 9440, bigint=True)
    case.check()
    case.close()


# ---- entry conventions ---------------------------------------------------------------------------------------------------------------
def _snapshot(polys):
    return [p.download().copy() for p in polys]


def test_rejections_leave_every_operand_unchanged(ctx):
    case = LeafCase(ctx, 8, "hiIdD", 7, 2, 9500)
    n = len(case.plan.leaves)
    assert A.ROWS["he_polyeval_leaves"].allowed == set()
    outs = case.outs()
    for o in outs:
        for p in o:
            p.upload(np.stack([Bd.word_row("uniform", case.rng, m, case.N) for m in case.q[: p.n_limbs]])[None].repeat(case.B, 0))
    xs = [p for k in sorted(case.X) for p in case.X[k]]
    everything = xs + [p for o in outs for p in o]
    before = _snapshot(everything)

    def rejected(call, code=-1):
        with pytest.raises(_lib.HeringError) as e:
            call()
        assert e.value.code == code, e.value
        ctx.sync()
        assert all(np.array_equal(a, b) for a, b in zip(_snapshot(everything), before))

    # every (output, power) pair, and two outputs that are one polynomial
    for g in range(n):
        for c in range(len(outs[g])):
            for x in xs:
                if x.n_limbs < case.plan.leaves[g][1] + 1:
                    continue
                alias = [list(o) for o in outs]
                alias[g][c] = x
                rejected(lambda: case.run(1, outs=alias))
    alias = [list(o) for o in outs]
    alias[1][0] = outs[0][0]
    rejected(lambda: case.run(1, outs=alias))
    alias = [list(o) for o in outs]
    alias[0][1] = outs[0][0]
    rejected(lambda: case.run(2, outs=alias))
    # a component too many, a component missing, too few limbs, another batch, a power that is not there
    rejected(lambda: case.run(1, outs=[o + [la.Poly(case.ring, case.level + 1, case.B)] for o in outs]))
    rejected(lambda: case.run(1, outs=[o[:1] for o in outs]))
    rejected(lambda: case.run(1, outs=[[la.Poly(case.ring, 1, case.B), o[1]] for o in outs]))
    rejected(lambda: case.run(1, outs=[[la.Poly(case.ring, case.level + 1, case.B + 1), o[1]] for o in outs]))
    keep = case.X.pop(2)
    case.X[2] = []
    rejected(lambda: case.run(1))
    case.X[2] = keep
    rejected(lambda: case.run(1, first=n - 1, count=2, outs=[outs[n - 1], outs[0]]))
    with pytest.raises(_lib.HeringError):
        case.run(3)
    # the caller's list against the decomposition, through the ring this time
    plan = case.plan
    ints = lambda v: (C.c_int * len(v))(*v)
    h = _lib.H()
    bad_level = [f[1] for f in plan.leaves]
    bad_level[0] += 1
    rc = _lib.load().he_polyeval_poly_create(case.ring.h, 7, 0, 1, 1, 0, 1, ints([1, case.level, 1]), n, ints([f[0] for f in plan.leaves]), ints(bad_level),
                                             case.s0.ctypes.data_as(_lib.u64p), case.s1.ctypes.data_as(_lib.u64p), C.byref(h))
    assert rc == -1 and b"is at level" in _lib.load().he_last_error()
    big = case.s0.copy()
    big[0][0] = case.q[0]
    rc = _lib.load().he_polyeval_poly_create(case.ring.h, 7, 0, 1, 1, 0, 1, ints([1, case.level, 1]), n, ints([f[0] for f in plan.leaves]),
                                             ints([f[1] for f in plan.leaves]), big.ctypes.data_as(_lib.u64p), case.s1.ctypes.data_as(_lib.u64p), C.byref(h))
    assert rc == -1 and b"not below the modulus" in _lib.load().he_last_error()
    case.check((1,))  # and the handle still works
    case.close()


def test_graph_capture_and_launch(ctx):
    case = LeafCase(ctx, 9, "dhiDIh", 17, 2, 9600)
    want = case.composed()
    outs = case.outs()
    case.run(2, outs=outs)
    ctx.sync()
    for o in outs:
        for p in o:
            p.Zero()
    with ctx.capture() as g:
        case.run(2, outs=outs)
    g.launch()
    ctx.sync()
    for o, w in zip(outs, want):
        assert np.array_equal(np.stack([p.download() for p in o], axis=1), w)
    case.close()


@pytest.mark.parametrize("deferred", [0, 4])
def test_queue_coalesced_and_deferred(ctx, deferred):
    """4 threads on their own batch-1 outputs; bit-identical to the direct calls (the requests are served one by one)"""
    case = LeafCase(ctx, 9, "dhiDIh", 17, 1, 9700 + deferred)
    want = case.composed()
    TH = 4
    outs = [case.outs() for _ in range(TH)]
    ctx.SetCoalescing(64, 2000)
    if deferred:
        ctx.SetDeferred(deferred)
    try:
        s0 = ctx.CoalescingStats()
        barrier, errs = threading.Barrier(TH), []

        def worker(t):
            try:
                barrier.wait()
                for _ in range(2):
                    case.run(0, outs=outs[t])
            except Exception as e:  # noqa: BLE001
                errs.append(e)
                barrier.abort()

        th = [threading.Thread(target=worker, args=(t,)) for t in range(TH)]
        [x.start() for x in th]
        [x.join() for x in th]
        ctx.sync()
        assert not errs, errs
        s1 = ctx.CoalescingStats()
    finally:
        if deferred:
            ctx.SetDeferred(0)
        ctx.SetCoalescing(0, 0)
    for t in range(TH):
        for o, w in zip(outs[t], want):
            assert np.array_equal(np.stack([p.download() for p in o], axis=1), w), t
    assert s1["calls"] - s0["calls"] == TH * 2, (s0, s1)
    case.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_bgv_degree_seven_decrypts_to_the_polynomial(ctx):
    """encrypt (host fixtures, a real secret and relinearization key) -> Evaluate of the shipped mirror (one native call) -> decrypt: p(m) in Z_t[X]/(X^N + 1) exactly.  tests/test_polyeval_host.py checks without a device that the oracle's own
    evaluation on this chain decrypts correctly."""
    from tests.gpu_common import Pair
    from tests.rlwe_fixtures import SecretKey, bgv_decrypt, bgv_encrypt, gen_evaluation_key, negacyclic_mul_mod
    logN = 9
    N = 1 << logN
    q, p = O.GenModuli(logN + 1, [55] + [45] * 7, [55, 55])
    pr = Pair(ctx, logN, len(q), len(p), qmods=q, pmods=p)
    rng = rng_for(9800)
    sk = SecretKey(rng, pr.oQ, pr.oP)
    rlk = gen_evaluation_key(rng, pr.oQ, pr.oP, pr.oQ.binop("MulCoeffsMontgomery", sk.Q, sk.Q), sk)
    gev = la.Evaluator(pr.gQ, pr.gP)
    gbe = S.BGVCiphertextEvaluator(gev, T, gev.NewEvaluationKey(rlk.q, rlk.p))
    m = rng.integers(0, T, size=N)
    coeffs = [int(x) for x in rng.integers(1, T, size=8)]
    ct = np.stack(list(bgv_encrypt(rng, pr.oQ, sk, m, T, 3)))
    gct = S.Ciphertext([la.Poly(pr.gQ, len(q), 1).upload(ct[k][None]) for k in range(2)], len(q) - 1, 3)
    me = NP.Evaluator(gev, NP.BGVScheme(q, T), gev.NewEvaluationKey(rlk.q, rlk.p))
    res = me.Evaluate(NP.Ciphertext(gct.Value, gct.level, 3), NP.Polynomial(coeffs), 11)  # ONE native call: he_polyeval_evaluate
    drv = NativeLeaves(gbe, pr.gQ).Evaluate(gct, driver_poly("bgv", coeffs, "Monomial", "both", False), 11)
    assert np.array_equal(words_of(res)[:, :, : res.level + 1], words_of(drv)[:, :, : drv.level + 1])
    words = np.stack([v.download()[0][: res.level + 1] for v in res.Value])
    got = bgv_decrypt(O.Ring(N, q[: res.level + 1]), words, sk, T, res.Scale)
    acc = np.zeros(N, dtype=np.int64)
    for c in reversed(coeffs):
        acc = negacyclic_mul_mod(acc, m, T)
        acc[0] = (acc[0] + c) % T
    assert res.Scale == 11 and np.array_equal(got, acc)



def test_native_evaluate_graph_capture_and_launch(ctx):
    """he_polyeval_evaluate recorded once and replayed (last in this file: the warm call before it leaves every buffer the
    recording takes in the context's cache)"""
    rg = Rig(ctx, 10, [55] + [45] * 7, [55, 55], 9990)
    rg.keys([1])
    me, gbe, obe, scale, target = mirror(rg, "bgv")
    pol = NP.Polynomial(coeffs_for("bgv", rg.rng, 7, "Monomial", "both"))
    gct = NP.Ciphertext(rg.up(rg.ct(7, 2)), 7, scale)
    want = words_of(me.Evaluate(gct, pol, target))
    me.Evaluate(gct, pol, target)
    ctx.sync()
    with ctx.capture() as g:
        res = me.Evaluate(gct, pol, target)
    for p in res.Value:
        p.Zero()
    g.launch()
    ctx.sync()
    assert np.array_equal(words_of(res), want)
