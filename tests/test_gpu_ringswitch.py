"""Ring-degree switching and rlwe.Evaluator.ApplyEvaluationKey on the device (include/hering_ringswitch.h), word for word
against the reference's own sequence of calls composed from the oracle: INTT at N -> keep every gap-th coefficient -> NTT at n
(core/rlwe/element.go:250-313), replication (ring/operations.go:380) and GadgetProduct + Add + Copy (applyEvaluationKey,
core/rlwe/evaluator_evaluationkey.go:98-106)."""
import threading

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd import _lib
from lattigo_amd import ring as G
from lattigo_amd import rlwe as R
from oracle import oracle as O
from tests.gpu_common import ctx  # noqa: F401
from tests.helpers import rng_for, uniform_poly
from tests.ringmap_ref import ref_down_ntt, ref_up_ntt  # (SwitchCiphertextRingDegreeNTT and the replication, on the oracle)
from tests.rlwe_fixtures import SecretKey, gen_evaluation_key, phase, small_to_rns

pytestmark = pytest.mark.gpu

C5_LOGQ = [60] + [40] * 9 + [39] * 3 + [60] * 8 + [56] * 4  # the c5 shape: 25 Q moduli, 5 P moduli
C5_LOGP = [61] * 5


# ---- the reference's sequences of calls, on the oracle ------------------------------------------------------------------------
def ref_apply(oev, oQ, level, ct, oevk, ci):
    """applyEvaluationKey at the evaluator's degree: GadgetProduct(ct[1]) -> (Add(ct[0], .[0]), .[1])"""
    gp = oev.GadgetProduct(level, ct[1][: level + 1], oevk)
    sub = O.Ring(oQ.N, oQ.moduli[: level + 1], ci)
    return np.stack([sub.binop("Add", ct[0][: level + 1], gp[0]), gp[1]])


def _moduli(log_nth, nq, np_=0, bits_q=55, bits_p=61):
    q, p = O.GenModuli(log_nth, [bits_q] * nq, [bits_p] * np_)
    return list(q), list(p)


def _rand(rng, q, N, batch):
    a = np.stack([uniform_poly(rng, q, N) for _ in range(batch)])
    return a if batch > 1 else a[0]


# ---- ring-level maps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [False, True])
@pytest.mark.parametrize("logn,logN", [(11, 12), (14, 16), (15, 16), (4, 8), (4, 12)])
def test_ring_level_maps(ctx, logn, logN, ci):
    n, N, gap = 1 << logn, 1 << logN, 1 << (logN - logn)
    q, _ = _moduli(logN + 2, 3)
    rng = rng_for(7100 + 10 * logN + logn + 1000 * ci)
    gbig, gsmall = la.Ring(ctx, N, q, conjugate_invariant=ci), la.Ring(ctx, n, q, conjugate_invariant=ci)
    for level in (2, 1):
        for batch in (1, 3):
            big = np.stack([uniform_poly(rng, q, N) for _ in range(batch)])
            if level == 2 and batch == 3:  # every word q - 1: the fold's accumulator at its largest
                big[1] = np.array([[qi - 1] * N for qi in q], dtype=np.uint64)
            small = np.stack([uniform_poly(rng, q, n) for _ in range(batch)])
            pbig = la.Poly(gbig, len(q), batch).upload(big)
            psmall = la.Poly(gsmall, len(q), batch).upload(small)
            # NTT domain, large -> small
            pre_s = np.stack([uniform_poly(rng, q, n) for _ in range(batch)])
            out = la.Poly(gsmall, len(q), batch).upload(pre_s)
            if level == 2:
                R.SwitchCiphertextRingDegreeNTT([pbig], gbig, [out])
            else:
                check(_lib.load().he_switch_ring_degree_ntt(gbig.h, level, pbig.h, out.h))
            got = out.download()
            for b in range(batch):
                assert np.array_equal(got[b, : level + 1], ref_down_ntt(big[b, : level + 1], q, N, gap, ci)), ("down ntt", level, b)
                assert np.array_equal(got[b, level + 1:], pre_s[b, level + 1:]), "limbs above level untouched"
            # NTT domain, small -> large (both entry points)
            outl = la.Poly(gbig, len(q), batch)
            check(_lib.load().he_switch_ring_degree_ntt(0, level, psmall.h, outl.h))
            got = outl.download()
            outm = la.Poly(gbig, level + 1, batch)
            G.MapSmallDimensionToLargerDimensionNTT(psmall, outm)
            for b in range(batch):
                assert np.array_equal(got[b, : level + 1], ref_up_ntt(small[b, : level + 1], gap)), ("up ntt", level, b)
            assert np.array_equal(outm.download(), got[:, : level + 1])
            # coefficient domain, down
            outc = la.Poly(gsmall, len(q), batch)
            check(_lib.load().he_switch_ring_degree(level, pbig.h, outc.h))
            got = outc.download()
            assert np.array_equal(got[:, : level + 1], big[:, : level + 1, ::gap])
            # coefficient domain, up: the words between the multiples of gap keep their pre-call values
            pre = np.stack([uniform_poly(rng, q, N) for _ in range(batch)])
            outu = la.Poly(gbig, len(q), batch).upload(pre)
            check(_lib.load().he_switch_ring_degree(level, psmall.h, outu.h))
            want = pre.copy()
            want[:, : level + 1, ::gap] = small[:, : level + 1]
            assert np.array_equal(outu.download(), want)
    ctx.sync()


def check(rc):
    _lib.check(rc)


# ---- ApplyEvaluationKey with random key words ------------------------------------------------------------------------------------
def _random_key(rng, q, p, N, level_q, pw2=0):
    if pw2:
        nj = [(int(x).bit_length() + pw2 - 1) // pw2 for x in q]
        D = sum(nj)
    else:
        nj, D = None, O.BaseRNSDecompositionVectorSize(len(q) - 1, len(p) - 1)
    kq = np.stack([np.stack([uniform_poly(rng, q, N) for _ in range(2)]) for _ in range(D)])
    kp = np.stack([np.stack([uniform_poly(rng, p, N) for _ in range(2)]) for _ in range(D)]) if p else \
        np.zeros((D, 2, 0, N), dtype=np.uint64)
    return kq, kp, nj


def _apply_case(ctx, logN, logn, q, p, pw2, ci, seed, forms=("same", "down", "up"), aliasing=True, batches=(1, 2)):
    N, n, gap = 1 << logN, 1 << logn, 1 << (logN - logn)
    rng = rng_for(seed)
    gQ, gP = la.Ring(ctx, N, q, conjugate_invariant=ci), la.Ring(ctx, N, p, conjugate_invariant=ci)
    gq_small = la.Ring(ctx, n, q, conjugate_invariant=ci)
    oQ, oP = O.Ring(N, q, ci), O.Ring(N, p, ci)
    gev, oev = la.Evaluator(gQ, gP), O.Evaluator(oQ, oP)
    kq, kp, nj = _random_key(rng, q, p, N, len(q) - 1, pw2)
    gk = gev.NewEvaluationKey(kq, kp, pw2, nj) if pw2 else gev.NewEvaluationKey(kq, kp)
    ok = O.EvaluationKey(kq, kp, pw2=pw2, nj=nj) if pw2 else O.EvaluationKey(kq, kp)
    nq = len(q)
    for level in (nq - 1, nq - 2):
        for batch in batches:
            big = [_rand(rng, q, N, batch) for _ in range(2)]
            small = [_rand(rng, q, n, batch) for _ in range(2)]
            ents = lambda a, b: a[b] if batch > 1 else a
            if "same" in forms:
                want = [ref_apply(oev, oQ, level, [ents(big[0], b), ents(big[1], b)], ok, ci) for b in range(batch)]
                pats = ["out"] + (["in-place", "crossed", "out0=in1", "out1=in1"] if aliasing and batch == 1 else [])
                for pat in pats:
                    i0, i1 = la.Poly(gQ, nq, batch).upload(big[0]), la.Poly(gQ, nq, batch).upload(big[1])
                    if pat == "out":
                        o = [la.Poly(gQ, nq, batch), la.Poly(gQ, nq, batch)]
                    elif pat == "in-place":
                        o = [i0, i1]
                    elif pat == "crossed":
                        o = [i1, i0]
                    elif pat == "out0=in1":
                        o = [i1, la.Poly(gQ, nq, batch)]
                    else:
                        o = [la.Poly(gQ, nq, batch), i1]
                    gev.ApplyEvaluationKey(level, [i0, i1], gk, o)
                    for k in range(2):
                        g = o[k].download()
                        for b in range(batch):
                            assert np.array_equal(g[b, : level + 1], want[b][k]), ("same", pat, level, batch, b, k)
            if "down" in forms:
                i0, i1 = la.Poly(gQ, nq, batch).upload(big[0]), la.Poly(gQ, nq, batch).upload(big[1])
                o = [la.Poly(gq_small, nq, batch), la.Poly(gq_small, nq, batch)]
                gev.ApplyEvaluationKey(level, [i0, i1], gk, o)
                for b in range(batch):
                    t = ref_apply(oev, oQ, level, [ents(big[0], b), ents(big[1], b)], ok, ci)
                    for k in range(2):
                        assert np.array_equal(o[k].download()[b, : level + 1], ref_down_ntt(t[k], q, N, gap, ci)), ("down", level, b, k)
                assert np.array_equal(i0.download().reshape(big[0].shape), big[0]), "inputs unchanged"
                assert np.array_equal(i1.download().reshape(big[1].shape), big[1]), "inputs unchanged"
            if "up" in forms:
                i0, i1 = la.Poly(gq_small, nq, batch).upload(small[0]), la.Poly(gq_small, nq, batch).upload(small[1])
                o = [la.Poly(gQ, nq, batch), la.Poly(gQ, nq, batch)]
                gev.ApplyEvaluationKey(level, [i0, i1], gk, o)
                for b in range(batch):
                    up = [ref_up_ntt(ents(small[k], b), gap) for k in range(2)]
                    t = ref_apply(oev, oQ, level, up, ok, ci)
                    for k in range(2):
                        assert np.array_equal(o[k].download()[b, : level + 1], t[k]), ("up", level, b, k)
    ctx.sync()


@pytest.mark.parametrize("ci", [False, True])
@pytest.mark.parametrize("logN,logn", [(12, 11), (13, 11)])
@pytest.mark.parametrize("gadget", ["multiP", "singleP", "base2"])
def test_apply_evaluation_key_random_keys(ctx, logN, logn, gadget, ci):
    np_ = {"multiP": 3, "singleP": 1, "base2": 1}[gadget]
    q, p = _moduli(logN + 2, 6, np_, bits_q=50, bits_p=55 if gadget != "base2" else 61)
    _apply_case(ctx, logN, logn, q, p, 20 if gadget == "base2" else 0, ci, 7300 + logN + 10 * logn + 100 * np_ + 1000 * ci)


def test_apply_evaluation_key_c5_moduli(ctx):
    """16 <-> 15 with the c5 shape's 25 + 5 moduli (the fused key-switch pipelines at full size), batch 1"""
    q, p = O.GenModuli(17, C5_LOGQ, C5_LOGP)
    _apply_case(ctx, 16, 15, list(q), list(p), 0, False, 7400, aliasing=False, batches=(1,))


@pytest.mark.parametrize("ci", [False, True])
def test_apply_evaluation_key_coefficient_domain(ctx, ci):
    """isNTT = False (composed on the host): the reference's coefficient-domain sequence -- SwitchCiphertextRingDegree before (n -> N,
    writing only the multiples of gap into opOut) or after (N -> n) the key switch, GadgetProduct + Add in the coefficient domain"""
    logN, logn = 12, 11
    N, n, gap = 1 << logN, 1 << logn, 1 << (logN - logn)
    q, p = _moduli(logN + 2, 4, 2, bits_q=50)
    rng = rng_for(7350 + ci)
    gQ, gP, gs = la.Ring(ctx, N, q, conjugate_invariant=ci), la.Ring(ctx, N, p, conjugate_invariant=ci), la.Ring(ctx, n, q, conjugate_invariant=ci)
    oQ, oP = O.Ring(N, q, ci), O.Ring(N, p, ci)
    gev, oev = la.Evaluator(gQ, gP), O.Evaluator(oQ, oP)
    kq, kp, _ = _random_key(rng, q, p, N, len(q) - 1)
    gk, ok = gev.NewEvaluationKey(kq, kp), O.EvaluationKey(kq, kp)
    level = len(q) - 1
    coeff = lambda ct: np.stack([oQ.INTT(c) for c in ct])
    ntt = lambda ct: np.stack([oQ.NTT(c) for c in ct])
    big = [uniform_poly(rng, q, N) for _ in range(2)]
    small = [uniform_poly(rng, q, n) for _ in range(2)]
    same = coeff(ref_apply(oev, oQ, level, ntt(big), ok, ci))
    # same degree
    o = [la.Poly(gQ, len(q)), la.Poly(gQ, len(q))]
    gev.ApplyEvaluationKey(level, [la.Poly(gQ, len(q)).upload(x) for x in big], gk, o, isNTT=False)
    assert all(np.array_equal(o[k].get(), same[k]) for k in range(2))
    # N -> n: key switch, then every gap-th coefficient
    o = [la.Poly(gs, len(q)), la.Poly(gs, len(q))]
    gev.ApplyEvaluationKey(level, [la.Poly(gQ, len(q)).upload(x) for x in big], gk, o, isNTT=False)
    assert all(np.array_equal(o[k].get(), same[k][:, ::gap]) for k in range(2))
    # n -> N: opOut's words between the multiples of gap take part, as in the reference
    pre = [uniform_poly(rng, q, N) for _ in range(2)]
    up = [x.copy() for x in pre]
    for k in range(2):
        up[k][:, ::gap] = small[k]
    want = coeff(ref_apply(oev, oQ, level, ntt(up), ok, ci))
    o = [la.Poly(gQ, len(q)).upload(x) for x in pre]
    gev.ApplyEvaluationKey(level, [la.Poly(gs, len(q)).upload(x) for x in small], gk, o, isNTT=False)
    assert all(np.array_equal(o[k].get(), want[k]) for k in range(2))


# ---- launch profile and accounting -----------------------------------------------------------------------------------------------
def _counted(ctx, call):
    """(alg_bytes, alg_valu) of one call, and nothing else"""
    ctx.alg_bytes(reset=True), ctx.alg_valu(reset=True)
    check(call())
    return ctx.alg_bytes(reset=True), ctx.alg_valu(reset=True)


def _profiled(ctx, call):
    """{kernel: (launches, algorithmic bytes)} of one call after a warm-up (plans and the arena are built on first use)"""
    check(call())
    ctx.sync()
    ctx.prof_begin()
    check(call())
    ctx.sync()
    return {k: (v[0], v[2]) for k, v in ctx.prof_end_bytes().items()}


MAP_KERNELS = ("ring_degree_fold_ntt", "ring_degree_replicate_ntt", "ring_degree_stride")


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("logn", [11, 10])
def test_degree_changing_forms_are_the_key_switch_plus_one_map(ctx, logn, batch):
    """large -> small at gap 2 and 4 and small -> large: the launches and counters of the same-degree he_apply_evaluation_key at
    that shape and level (measured here) plus exactly one map launch over both components -- N + n words per limb and entry, moved
    and charged; the fold one integer product per output word on top"""
    logN = 12
    N, n, gap = 1 << logN, 1 << logn, 1 << (logN - logn)
    q, p = _moduli(logN + 2, 6, 3, bits_q=50, bits_p=55)
    rng = rng_for(7500 + 10 * logn + batch)
    gQ, gP, gs = la.Ring(ctx, N, q), la.Ring(ctx, N, p), la.Ring(ctx, n, q)
    gev = la.Evaluator(gQ, gP)
    kq, kp, _ = _random_key(rng, q, p, N, len(q) - 1)
    gk = gev.NewEvaluationKey(kq, kp)
    nq, level = len(q), len(q) - 2
    L = level + 1
    big = [la.Poly(gQ, nq, batch).upload(_rand(rng, q, N, batch)) for _ in range(4)]
    small = [la.Poly(gs, nq, batch).upload(_rand(rng, q, n, batch)) for _ in range(4)]
    lib = _lib.load()
    calls = {
        "same": lambda: lib.he_apply_evaluation_key(gev.h, level, big[0].h, big[1].h, gk.h, big[2].h, big[3].h),
        "down": lambda: lib.he_apply_evaluation_key(gev.h, level, big[0].h, big[1].h, gk.h, small[2].h, small[3].h),
        "up": lambda: lib.he_apply_evaluation_key(gev.h, level, small[0].h, small[1].h, gk.h, big[2].h, big[3].h),
    }
    prof = {name: _profiled(ctx, call) for name, call in calls.items()}
    acct = {name: _counted(ctx, call) for name, call in calls.items()}
    print(prof, acct)
    assert not any(k in prof["same"] for k in MAP_KERNELS)
    map_bytes = float((N + n) * L * 2 * batch * 8)
    for name, kernel in (("down", "ring_degree_fold_ntt"), ("up", "ring_degree_replicate_ntt")):
        got = dict(prof[name])
        assert got.pop(kernel) == (1, map_bytes), (name, prof[name])
        assert not any(k in got for k in MAP_KERNELS), (name, prof[name])
        assert got == prof["same"], (name, got, prof["same"])
        # charged: L (1 + 1/gap) limbs per component, no shared part
        assert 2 * L * (1 + 1 / gap) * batch * N * 8 == map_bytes
        (b0, b1), v = acct[name]
        (s0, s1), sv = acct["same"]
        assert (b0, b1) == (s0 + map_bytes, s1 + map_bytes), (name, acct[name], acct["same"])
        muls = 2 * L * n * batch if name == "down" else 0
        assert v == [sv[0] + muls, sv[1], sv[2], sv[3]], (name, v, sv)


@pytest.mark.parametrize("ci", [False, True])
def test_ring_level_maps_accounting(ctx, ci):
    """the counters of he_switch_ring_degree_ntt (both directions) and he_switch_ring_degree (both directions) in closed form:
    L (1 + 1/gap) limbs of N words for the fold and the replication, 2 L / gap for the strides, one product per word of the fold"""
    logN, logn, batch, level = 8, 6, 3, 1
    N, n, gap, L = 1 << logN, 1 << logn, 1 << (logN - logn), level + 1
    q, _ = _moduli(logN + 2, 3)
    rng = rng_for(7600 + ci)
    gbig, gsmall = la.Ring(ctx, N, q, conjugate_invariant=ci), la.Ring(ctx, n, q, conjugate_invariant=ci)
    pbig = la.Poly(gbig, len(q), batch).upload(np.stack([uniform_poly(rng, q, N) for _ in range(batch)]))
    psmall = la.Poly(gsmall, len(q), batch).upload(np.stack([uniform_poly(rng, q, n) for _ in range(batch)]))
    obig, osmall = la.Poly(gbig, len(q), batch), la.Poly(gsmall, len(q), batch)
    lib = _lib.load()
    ntt_bytes = float(L * (N + n) * batch * 8)
    assert L * (1 + 1 / gap) * batch * N * 8 == ntt_bytes
    stride_bytes = float(2 * L * n * batch * 8)
    zero = [0.0, 0.0, 0.0, 0.0]
    assert _counted(ctx, lambda: lib.he_switch_ring_degree_ntt(gbig.h, level, pbig.h, osmall.h)) == \
        ((ntt_bytes, ntt_bytes), [float(L * n * batch), 0.0, 0.0, 0.0])
    assert _counted(ctx, lambda: lib.he_switch_ring_degree_ntt(0, level, psmall.h, obig.h)) == ((ntt_bytes, ntt_bytes), zero)
    assert _counted(ctx, lambda: lib.he_map_small_to_large_ntt(psmall.h, obig.h, level)) == ((ntt_bytes, ntt_bytes), zero)
    assert _counted(ctx, lambda: lib.he_switch_ring_degree(level, pbig.h, osmall.h)) == ((stride_bytes, stride_bytes), zero)
    assert _counted(ctx, lambda: lib.he_switch_ring_degree(level, psmall.h, obig.h)) == ((stride_bytes, stride_bytes), zero)
    ctx.sync()


# ---- functional: real keys --------------------------------------------------------------------------------------------------------
def _functional_setup(ctx, logN, logn, seed):
    N, n, gap = 1 << logN, 1 << logn, 1 << (logN - logn)
    q, p = _moduli(logN + 1, 4, 2)
    rng = rng_for(seed)
    oQ, oP = O.Ring(N, q), O.Ring(N, p)
    oq_small = O.Ring(n, q)
    gQ, gP, gq_small = la.Ring(ctx, N, q), la.Ring(ctx, N, p), la.Ring(ctx, n, q)
    gev = la.Evaluator(gQ, gP)
    sk_large = SecretKey(rng, oQ, oP)
    sk_small_vals = rng.integers(-1, 2, size=n)
    sk_small = SecretKey(rng, O.Ring(n, q), O.Ring(n, p), vals=sk_small_vals)
    up_vals = np.zeros(N, dtype=np.int64)
    up_vals[::gap] = sk_small_vals  # the small secret mapped up: s(Y) with Y = X^gap
    sk_up = SecretKey(rng, oQ, oP, vals=up_vals)
    return dict(N=N, n=n, gap=gap, q=q, p=p, rng=rng, oQ=oQ, oP=oP, oq_small=oq_small, gQ=gQ, gP=gP, gq_small=gq_small, gev=gev,
                sk_large=sk_large, sk_small=sk_small, sk_up=sk_up)


def _encrypt_zero(rng, ring, skQ, level, sigma=3.2):
    """(-a s + e, a), NTT domain, limbs 0..level"""
    sub = O.Ring(ring.N, ring.moduli[: level + 1], getattr(ring, "conjugate_invariant", False))
    a = np.stack([rng.integers(0, int(x), size=ring.N, dtype=np.uint64) for x in sub.moduli])
    e = np.clip(np.rint(rng.normal(0.0, sigma, size=ring.N)), -19, 19).astype(np.int64)
    eN = sub.NTT(small_to_rns(e, sub.moduli))
    b = sub.binop("Sub", eN, sub.binop("MulCoeffsMontgomery", a, skQ[: level + 1]))
    return np.stack([b, a])


def _noise(ring, ct, skQ, level):
    """log2 of the standard deviation of the decrypted coefficients (ring.Ring.Log2OfStandardDeviation), limb 0"""
    sub = O.Ring(ring.N, ring.moduli[: level + 1], getattr(ring, "conjugate_invariant", False))
    c = sub.INTT(phase(ring, ct[:, : level + 1], skQ))[0]
    q0 = int(ring.moduli[0])
    v = np.array([int(x) - q0 if int(x) > q0 // 2 else int(x) for x in c], dtype=np.float64)
    return float(np.log2(np.std(v))) if np.std(v) > 0 else 0.0


@pytest.mark.parametrize("logN,logn", [(12, 11), (13, 11)])
def test_apply_evaluation_key_functional(ctx, logN, logn):
    """core/rlwe/rlwe_test.go:781-895: the same degree, n -> N and N -> n, each decrypting under the target key with noise below
    LogN + bpw2 (bpw2 = 0: RNS gadget); plus a message m(X^gap) encrypted at N decrypts to m at n and back."""
    S = _functional_setup(ctx, logN, logn, 7500 + logN + logn)
    N, n, gap, q, rng, oQ, oP, gev = S["N"], S["n"], S["gap"], S["q"], S["rng"], S["oQ"], S["oP"], S["gev"]
    gQ, gs = S["gQ"], S["gq_small"]
    level, bound = len(q) - 1, logN
    # same degree: skLarge -> sk2
    sk2 = SecretKey(rng, oQ, oP)
    k = gen_evaluation_key(rng, oQ, oP, S["sk_large"].Q, sk2)
    gk = gev.NewEvaluationKey(k.q, k.p)
    ct = _encrypt_zero(rng, oQ, S["sk_large"].Q, level)
    pc = [la.Poly(gQ, level + 1).upload(ct[i]) for i in range(2)]
    out = [la.Poly(gQ, level + 1), la.Poly(gQ, level + 1)]
    gev.ApplyEvaluationKey(level, pc, gk, out)
    assert _noise(oQ, np.stack([o.get() for o in out]), sk2.Q, level) <= bound
    # n -> N: key from the small secret (mapped up) to the large one
    k_up = gen_evaluation_key(rng, oQ, oP, S["sk_up"].Q, S["sk_large"])
    gk_up = gev.NewEvaluationKey(k_up.q, k_up.p)
    cts = _encrypt_zero(rng, S["oq_small"], S["sk_small"].Q, level)
    pcs = [la.Poly(gs, level + 1).upload(cts[i]) for i in range(2)]
    outL = [la.Poly(gQ, level + 1), la.Poly(gQ, level + 1)]
    gev.ApplyEvaluationKey(level, pcs, gk_up, outL)
    assert _noise(oQ, np.stack([o.get() for o in outL]), S["sk_large"].Q, level) <= bound
    # N -> n: key from the large secret to the small secret mapped up
    k_dn = gen_evaluation_key(rng, oQ, oP, S["sk_large"].Q, S["sk_up"])
    gk_dn = gev.NewEvaluationKey(k_dn.q, k_dn.p)
    outS = [la.Poly(gs, level + 1), la.Poly(gs, level + 1)]
    gev.ApplyEvaluationKey(level, pc, gk_dn, outS)
    assert _noise(S["oq_small"], np.stack([o.get() for o in outS]), S["sk_small"].Q, level) <= bound
    # m(X^gap) at N -> m at n, and m at n -> m(X^gap) at N (a message of a few bits over the noise)
    m = rng.integers(-8, 9, size=n) << 20
    mN = np.zeros(N, dtype=np.int64)
    mN[::gap] = m
    ctm = _encrypt_zero(rng, oQ, S["sk_large"].Q, level)
    ctm[0] = oQ.binop("Add", ctm[0], oQ.NTT(small_to_rns(mN, q)))
    pm = [la.Poly(gQ, level + 1).upload(ctm[i]) for i in range(2)]
    gev.ApplyEvaluationKey(level, pm, gk_dn, outS)
    dec = S["oq_small"].INTT(phase(S["oq_small"], np.stack([o.get() for o in outS]), S["sk_small"].Q))
    q0 = int(q[0])
    got = np.array([int(x) - q0 if int(x) > q0 // 2 else int(x) for x in dec[0]], dtype=np.int64)
    assert np.all(np.abs(got - m) < (1 << 19)), np.max(np.abs(got - m))
    ctsm = _encrypt_zero(rng, S["oq_small"], S["sk_small"].Q, level)
    ctsm[0] = S["oq_small"].binop("Add", ctsm[0], S["oq_small"].NTT(small_to_rns(m, q)))
    psm = [la.Poly(gs, level + 1).upload(ctsm[i]) for i in range(2)]
    gev.ApplyEvaluationKey(level, psm, gk_up, outL)
    dec = oQ.INTT(phase(oQ, np.stack([o.get() for o in outL]), S["sk_large"].Q))
    got = np.array([int(x) - q0 if int(x) > q0 // 2 else int(x) for x in dec[0]], dtype=np.int64)
    assert np.all(np.abs(got - mN) < (1 << 19)), np.max(np.abs(got - mN))


# ---- the submission queue, graphs and replay -------------------------------------------------------------------------------------
def _queue_setup(ctx, seed):
    logN, logn = 12, 11
    N, n = 1 << logN, 1 << logn
    q, p = _moduli(logN + 1, 5, 2)
    rng = rng_for(seed)
    gQ, gP, gs = la.Ring(ctx, N, q), la.Ring(ctx, N, p), la.Ring(ctx, n, q)
    gev = la.Evaluator(gQ, gP)
    kq, kp, _ = _random_key(rng, q, p, N, len(q) - 1)
    gk = gev.NewEvaluationKey(kq, kp)
    return rng, q, N, n, gQ, gs, gev, gk


def _direct(gev, gk, level, ins, outs):
    gev.ApplyEvaluationKey(level, ins, gk, outs)


def _op_stats(ctx):
    ops = np.zeros(64, dtype=np.uint64)
    _lib.check(_lib.load().he_debug_queue_op_stats(ctx.h, ops.ctypes.data_as(_lib.u64p)))
    return ops


CO_APPLY_EVK = 30  # (csrc/api.cpp, enum CoOp)


@pytest.mark.parametrize("deferred", [0, 4])
def test_queue_coalesced_and_deferred(ctx, deferred):
    """8 threads on their own batch-1 handles, each form in turn; bit-identical to the direct calls; the same-degree form ran
    batched (fewer launches than calls)"""
    rng, q, N, n, gQ, gs, gev, gk = _queue_setup(ctx, 7600 + deferred)
    level, T, REP = len(q) - 1, 8, 3
    forms = {"same": (gQ, gQ), "down": (gQ, gs), "up": (gs, gQ)}
    for f, (gi, go) in forms.items():
        data = [[uniform_poly(rng, q, gi.N) for _ in range(2)] for _ in range(T)]
        want = []
        for t in range(T):
            ins = [la.Poly(gi, len(q)).upload(x) for x in data[t]]
            outs = [la.Poly(go, len(q)), la.Poly(go, len(q))]
            _direct(gev, gk, level, ins, outs)
            want.append([o.get() for o in outs])
        ctx.sync()
        ins = [[la.Poly(gi, len(q)).upload(x) for x in data[t]] for t in range(T)]
        outs = [[la.Poly(go, len(q)), la.Poly(go, len(q))] for _ in range(T)]
        ctx.SetCoalescing(64, 2000)
        if deferred:
            ctx.SetDeferred(deferred)
        try:
            s0, o0 = ctx.CoalescingStats(), _op_stats(ctx)
            barrier, errs = threading.Barrier(T), []

            def worker(t):
                try:
                    barrier.wait()
                    for _ in range(REP):
                        _direct(gev, gk, level, ins[t], outs[t])
                except Exception as e:  # noqa: BLE001
                    errs.append(e)
                    barrier.abort()

            th = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
            [x.start() for x in th]
            [x.join() for x in th]
            ctx.sync()
            assert not errs, errs
            s1, o1 = ctx.CoalescingStats(), _op_stats(ctx)
        finally:
            if deferred:
                ctx.SetDeferred(0)
            ctx.SetCoalescing(0, 0)
        for t in range(T):
            for k in range(2):
                assert np.array_equal(outs[t][k].get(), want[t][k]), (f, t, k)
        launches = int(o1[2 * CO_APPLY_EVK]) - int(o0[2 * CO_APPLY_EVK])
        calls = int(o1[2 * CO_APPLY_EVK + 1]) - int(o0[2 * CO_APPLY_EVK + 1])
        assert calls == T * REP, (f, calls)
        if f == "same":
            assert launches < calls, (launches, calls)
            assert s1["launches"] - s0["launches"] < s1["calls"] - s0["calls"], (s0, s1)


def test_graph_replays_large_to_small(ctx):
    rng, q, N, n, gQ, gs, gev, gk = _queue_setup(ctx, 7700)
    level = len(q) - 1
    x = [uniform_poly(rng, q, N) for _ in range(2)]
    ins = [la.Poly(gQ, len(q)).upload(v) for v in x]
    outs = [la.Poly(gs, len(q)), la.Poly(gs, len(q))]
    gev.ApplyEvaluationKey(level, ins, gk, outs)  # (plans and the arena are built on first use)
    want = [o.get() for o in outs]
    for o in outs:
        o.Zero()
    with ctx.capture() as g:
        gev.ApplyEvaluationKey(level, ins, gk, outs)
    g.launch()
    ctx.sync()
    assert all(np.array_equal(o.get(), w) for o, w in zip(outs, want))


def test_trace_replay_of_the_three_forms(ctx):
    rng, q, N, n, gQ, gs, gev, gk = _queue_setup(ctx, 7800)
    level = len(q) - 1
    forms = [(gQ, gQ), (gQ, gs), (gs, gQ)]
    ins = [[la.Poly(gi, len(q)).upload(uniform_poly(rng, q, gi.N)) for _ in range(2)] for gi, _ in forms]
    outs = [[la.Poly(go, len(q)), la.Poly(go, len(q))] for _, go in forms]
    for i in range(3):
        _direct(gev, gk, level, ins[i], outs[i])
    R.SwitchCiphertextRingDegreeNTT(outs[2], gQ, outs[1])
    R.SwitchCiphertextRingDegree(outs[1], outs[2])
    G.MapSmallDimensionToLargerDimensionNTT(outs[1][0], outs[0][1])
    ctx.sync()
    want = [[o.get() for o in oo] for oo in outs]
    for oo in outs:
        for o in oo:
            o.Zero()
    _lib.trace_begin()
    try:
        for i in range(3):
            _direct(gev, gk, level, ins[i], outs[i])
        R.SwitchCiphertextRingDegreeNTT(outs[2], gQ, outs[1])
        R.SwitchCiphertextRingDegree(outs[1], outs[2])
        G.MapSmallDimensionToLargerDimensionNTT(outs[1][0], outs[0][1])
    finally:
        prog = _lib.trace_end()
    ctx.sync()
    for oo in outs:
        for o in oo:
            o.Zero()
    ctx.sync()
    _lib.replay(ctx.h, prog, 1, 1, [], [], [])
    ctx.sync()
    for i in range(3):
        for k in range(2):
            assert np.array_equal(outs[i][k].get(), want[i][k]), (i, k)


# ---- equal degrees: the maps are copies, onto their own input no-ops (include/hering_ringswitch.h) -------------------------------
@pytest.mark.parametrize("ci", [False, True])
def test_equal_degree_maps_copy_or_no_op(ctx, ci):
    N = 1 << 12
    q, _ = _moduli(14, 3)
    rng = rng_for(7950 + ci)
    g = la.Ring(ctx, N, q, conjugate_invariant=ci)
    L = _lib.load()
    x = np.stack([uniform_poly(rng, q, N) for _ in range(2)])
    calls = {
        "he_map_small_to_large_ntt": lambda a, b, lv: L.he_map_small_to_large_ntt(a.h, b.h, lv),
        "he_switch_ring_degree_ntt": lambda a, b, lv: L.he_switch_ring_degree_ntt(0, lv, a.h, b.h),
        "he_switch_ring_degree_ntt (ring)": lambda a, b, lv: L.he_switch_ring_degree_ntt(g.h, lv, a.h, b.h),
        "he_switch_ring_degree": lambda a, b, lv: L.he_switch_ring_degree(lv, a.h, b.h),
    }
    for name, call in calls.items():
        p = la.Poly(g, len(q), 2).upload(x)
        assert call(p, p, len(q) - 1) == 0, name
        ctx.sync()
        assert np.array_equal(p.download(), x), (name, "x onto x")
        pre = np.stack([uniform_poly(rng, q, N) for _ in range(2)])
        o = la.Poly(g, len(q), 2).upload(pre)
        assert call(p, o, 1) == 0, name
        want = pre.copy()
        want[:, :2] = x[:, :2]
        assert np.array_equal(o.download(), want), (name, "copy of limbs 0..level")
        assert np.array_equal(p.download(), x), (name, "input unchanged")


# ---- rejections ------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_every_operand_unchanged(ctx):
    rng, q, N, n, gQ, gs, gev, gk = _queue_setup(ctx, 7900)
    level = len(q) - 1
    g4k = la.Ring(ctx, N // 4, q)
    big = [la.Poly(gQ, len(q)).upload(uniform_poly(rng, q, N)) for _ in range(3)]
    small = [la.Poly(gs, len(q)).upload(uniform_poly(rng, q, n)) for _ in range(4)]
    other = la.Poly(g4k, len(q)).upload(uniform_poly(rng, q, N // 4))
    allp = big + small + [other]
    before = [p.download() for p in allp]
    L = _lib.load()
    EINVAL, EHANDLE = -1, -2
    cases = [
        (EINVAL, lambda: L.he_apply_evaluation_key(gev.h, level, big[0].h, big[1].h, gk.h, big[2].h, big[2].h)),    # out0 == out1
        (EINVAL, lambda: L.he_apply_evaluation_key(gev.h, level, big[0].h, big[1].h, gk.h, small[0].h, big[2].h)),  # components differ
        (EINVAL, lambda: L.he_apply_evaluation_key(gev.h, level, small[0].h, small[1].h, gk.h, other.h, other.h)),  # large side != N
        (EINVAL, lambda: L.he_apply_evaluation_key(gev.h, level, other.h, big[1].h, gk.h, small[0].h, small[1].h)), # degree mismatch
        (EINVAL, lambda: L.he_apply_evaluation_key(gev.h, level, small[0].h, small[1].h, gk.h, small[0].h, big[0].h)),
        (EINVAL, lambda: L.he_apply_evaluation_key(gev.h, level, small[0].h, small[1].h, gk.h, small[2].h, small[3].h)),  # all of degree n < N
        (EINVAL, lambda: L.he_apply_evaluation_key(gev.h, 0, small[0].h, small[1].h, gk.h, small[0].h, small[1].h)),    # the same, in place
        (EINVAL, lambda: L.he_map_small_to_large_ntt(big[0].h, small[0].h, level)),                                 # small > large
        (EINVAL, lambda: L.he_switch_ring_degree_ntt(g4k.h, level, big[0].h, small[0].h)),                          # ring degree
        (EHANDLE, lambda: L.he_switch_ring_degree_ntt(0, level, big[0].h, small[0].h)),                             # no ring for N -> n
        (EINVAL, lambda: L.he_switch_ring_degree(len(q), big[0].h, small[0].h)),                                    # level
    ]
    for i, (code, c) in enumerate(cases):
        assert c() == code, i
    with pytest.raises(la.HeringError):  # the Python mirror's coefficient-domain form rejects it before composing anything
        gev.ApplyEvaluationKey(level, small[:2], gk, small[2:], isNTT=False)
    # a degree below 16 cannot be formed: rings start at logN = 4 (he_ring_create), so no such polynomial reaches the entries
    with pytest.raises(la.HeringError):
        la.Ring(ctx, 8, q)
    ctx.sync()
    for p, b in zip(allp, before):
        assert np.array_equal(p.download(), b)
