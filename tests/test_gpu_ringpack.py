"""The ring-packing evaluator on the device (include/hering_ringpack.h, lattigo_amd.rlwe.RingPackingEvaluator), word for word
against tests/ringpack_ref.py -- core/rlwe/ring_packing.go restated on the oracle with materialised monomial tables -- at the
smallest shapes at which each path can still go wrong."""
import gc
import threading

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd import _lib
from lattigo_amd import rlwe as R
from oracle import oracle as O
from tests import ringpack_ref as REF
from tests.gpu_common import ctx  # noqa: F401
from tests.helpers import rng_for, uniform_poly

pytestmark = pytest.mark.gpu

C5_LOGQ = [60] + [40] * 9 + [39] * 3 + [60] * 8 + [56] * 4  # the c5 shape: 25 Q moduli, 5 P moduli
C5_LOGP = [61] * 5
EINVAL = -1


@pytest.fixture(autouse=True)
def _no_garbage_left_behind():
    """A la.Ring owns itself (Ring._owner), so the rings a test drops are released by the cycle collector, whenever it next runs.
    Collect them at the test's own boundaries: these tests make many rings, and the next one starts from a settled device."""
    gc.collect()
    yield
    gc.collect()


def _moduli(log_nth, logq, logp=()):
    q, p = O.GenModuli(log_nth, list(logq), list(logp))
    return list(q), list(p)


def _stack(rng, q, N, batch):
    return np.stack([uniform_poly(rng, q, N) for _ in range(batch)])


def _up(ring, arr):
    arr = np.asarray(arr, dtype=np.uint64)
    if arr.ndim == 2:
        arr = arr[None]
    return la.Poly(ring, arr.shape[1], arr.shape[0]).upload(arr)


def _up_ct(ring, ct, nlimbs=None):
    """[2][L][N] (one ciphertext) or [B][2][L][N] -> [Poly, Poly]"""
    ct = np.asarray(ct, dtype=np.uint64)
    if ct.ndim == 3:
        ct = ct[None]
    return [_up(ring, ct[:, k]) for k in range(2)]


def _down_ct(ct, level):
    """[Poly, Poly] -> [B][2][level + 1][N]"""
    return np.stack([c.download()[:, : level + 1] for c in ct], axis=1)


def _random_key(rng, q, p, N, pw2=0):
    if pw2:
        nj = [(int(x).bit_length() + pw2 - 1) // pw2 for x in q]
        D = sum(nj)
    else:
        nj, D = None, O.BaseRNSDecompositionVectorSize(len(q) - 1, len(p) - 1)
    kq = np.stack([np.stack([uniform_poly(rng, q, N) for _ in range(2)]) for _ in range(D)])
    kp = np.stack([np.stack([uniform_poly(rng, p, N) for _ in range(2)]) for _ in range(D)])
    return O.EvaluationKey(kq, kp, pw2=pw2, nj=nj) if pw2 else O.EvaluationKey(kq, kp)


def _device(ctx, rings, rsk=None, ext=None, rep=None):
    """the device twin of a REF.RingPackingEvaluator's rings and keys"""
    gr = {n: (la.Ring(ctx, 1 << n, rq.moduli), la.Ring(ctx, 1 << n, rp.moduli)) for n, (rq, rp) in rings.items()}
    gev = {n: la.Evaluator(*gr[n]) for n in gr}

    def up(n, k):
        return gev[n].NewEvaluationKey(k.q, k.p, k.pw2, k.nj) if k.pw2 else gev[n].NewEvaluationKey(k.q, k.p)
    RSK = {ab: up(max(ab), k) for ab, k in (rsk or {}).items()}
    EXT = {n: R.GaloisKeySet({g: up(n, k) for g, k in ks.items()}) for n, ks in ext.items()} if ext is not None else None
    REP = {n: R.GaloisKeySet({g: up(n, k) for g, k in ks.items()}) for n, ks in rep.items()} if rep is not None else None
    return R.RingPackingEvaluator(gev, RSK, REP, EXT), gr


# ---- 1. the monomial tables --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logN", [4, 5, 12, 13, 16])
def test_xpow2_ntt(ctx, logN):
    q, _ = _moduli(17, [60, 45])  # one generic modulus, one of the double-precision class
    N = 1 << logN
    g, o = la.Ring(ctx, N, q), O.Ring(N, q)
    rng = rng_for(8300 + logN)
    pre = _stack(rng, q, N, 2)
    for div in (False, True):
        want = REF.GenXPow2NTT(o, logN, div)
        for i in range(logN):
            out = la.Poly(g, 2, 1)
            R.XPow2NTT(g, 1, i, div, out)
            assert np.array_equal(out.get(), want[i]), (logN, i, div)
    # level 0 on a batch of two: limb 1 keeps its words, both entries are filled
    out = _up(g, pre)
    R.XPow2NTT(g, 0, logN - 1, True, out)
    got = out.download()
    for b in range(2):
        assert np.array_equal(got[b, 0], want[logN - 1][0]) and np.array_equal(got[b, 1], pre[b, 1])
    L = _lib.load()
    assert L.he_ring_xpow2_ntt(g.h, 1, logN, 0, out.h) == EINVAL and L.he_ring_xpow2_ntt(g.h, 1, -1, 0, out.h) == EINVAL
    assert L.he_ring_xpow2_ntt(g.h, 2, 0, 0, out.h) == EINVAL


# ---- 2. the ring maps of Split and Merge ------------------------------------------------------------------------------------------
def _ref_split_poly(o, t, xinv0):
    n = o.N // 2
    return REF.switch_down_ntt(t, o, n), REF.switch_down_ntt(o.binop("MulCoeffsMontgomery", t, xinv0[: t.shape[0]]), o, n)


def _ref_merge_poly(o, e, od, x0):
    out = REF.switch_up_ntt(e, 2)
    if od is None:
        return out
    sub = O.Ring(o.N, o.moduli[: e.shape[0]])
    return sub.binop("MulCoeffsMontgomeryThenAdd", REF.switch_up_ntt(od, 2), x0[: e.shape[0]], out)


@pytest.mark.parametrize("logN", [5, 12, 16])
def test_ring_split_and_merge_ntt(ctx, logN):
    q, _ = _moduli(17, [60, 45, 55])
    N, n = 1 << logN, 1 << (logN - 1)
    gN, gn, o = la.Ring(ctx, N, q), la.Ring(ctx, n, q), O.Ring(N, q)
    rng = rng_for(8400 + logN)
    xinv0, x0 = REF.GenXPow2NTT(o, 1, True)[0], REF.GenXPow2NTT(o, 1, False)[0]
    for level in (2, 1):
        for batch in (1, 3):
            big, ev, od = _stack(rng, q, N, batch), _stack(rng, q, n, batch), _stack(rng, q, n, batch)
            if batch == 3:  # one entry with every word q - 1
                big[1] = np.array([[qi - 1] * N for qi in q], dtype=np.uint64)
                ev[1] = od[1] = np.array([[qi - 1] * n for qi in q], dtype=np.uint64)
            sub = O.Ring(N, q[: level + 1])
            for with_odd in (True, False):
                pre = [_stack(rng, q, n, batch) for _ in range(2)]
                pin, pe, po = _up(gN, big), _up(gn, pre[0]), _up(gn, pre[1])
                R.SplitNTT(gN, level, pin, pe, po if with_odd else None)
                ge, go = pe.download(), po.download()
                for b in range(batch):
                    we, wo = _ref_split_poly(sub, big[b, : level + 1], xinv0)
                    assert np.array_equal(ge[b, : level + 1], we), ("even", logN, level, batch, b)
                    if with_odd:
                        assert np.array_equal(go[b, : level + 1], wo), ("odd", logN, level, batch, b)
                assert np.array_equal(ge[:, level + 1:], pre[0][:, level + 1:]), "limbs above level keep their words"
                assert np.array_equal(go[:, level + 1:], pre[1][:, level + 1:])
                if not with_odd:
                    assert np.array_equal(go, pre[1]), "the absent operand's polynomial is not written"
                assert np.array_equal(pin.download(), big), "input unchanged"
                preN = _stack(rng, q, N, batch)
                pout = _up(gN, preN)
                R.MergeNTT(gN, level, _up(gn, ev), _up(gn, od) if with_odd else None, pout)
                got = pout.download()
                for b in range(batch):
                    want = _ref_merge_poly(sub, ev[b, : level + 1], od[b, : level + 1] if with_odd else None, x0)
                    assert np.array_equal(got[b, : level + 1], want), ("merge", logN, level, batch, b, with_odd)
                assert np.array_equal(got[:, level + 1:], preN[:, level + 1:])
    ctx.sync()


# ---- 3. Split / Merge with random key words ----------------------------------------------------------------------------------------
def _split_merge_case(ctx, logN, q, p, pw2, seed, batches=(1, 2), levels=None):
    N, n = 1 << logN, 1 << (logN - 1)
    rng = rng_for(seed)
    rings = {logN - 1: (O.Ring(n, q), O.Ring(n, p)), logN: (O.Ring(N, q), O.Ring(N, p))}
    rsk = {(logN, logN - 1): _random_key(rng, q, p, N, pw2), (logN - 1, logN): _random_key(rng, q, p, N, pw2)}
    ref = REF.RingPackingEvaluator(rings, rsk)
    dev, gr = _device(ctx, rings, rsk)
    nq = len(q)
    for level in levels or (nq - 1, nq - 2):
        for batch in batches:
            big = np.stack([np.stack([uniform_poly(rng, q, N) for _ in range(2)]) for _ in range(batch)])
            ctN = _up_ct(gr[logN][0], big)
            even, odd = dev.SplitNew(level, ctN)
            ge, go = _down_ct(even, level), _down_ct(odd, level)
            even_only = dev.NewCiphertext(logN - 1, level, batch)
            dev.Split(level, ctN, even_only)
            for b in range(batch):
                we, wo = ref.Split(big[b][:, : level + 1])
                assert np.array_equal(ge[b], we), ("split even", logN, level, batch, b)
                assert np.array_equal(go[b], wo), ("split odd", logN, level, batch, b)
            assert np.array_equal(_down_ct(even_only, level), ge), "Split without the odd half"
            assert np.array_equal(_down_ct(ctN, nq - 1), big), "inputs unchanged"
            halves = [np.stack([np.stack([uniform_poly(rng, q, n) for _ in range(2)]) for _ in range(batch)]) for _ in range(2)]
            ce, co = _up_ct(gr[logN - 1][0], halves[0]), _up_ct(gr[logN - 1][0], halves[1])
            gm = _down_ct(dev.MergeNew(level, ce, co), level)
            gm1 = _down_ct(dev.MergeNew(level, ce, None), level)
            for b in range(batch):
                assert np.array_equal(gm[b], ref.Merge(halves[0][b][:, : level + 1], halves[1][b][:, : level + 1])), ("merge", logN, level, b)
                assert np.array_equal(gm1[b], ref.Merge(halves[0][b][:, : level + 1], None)), ("merge, even only", logN, level, b)
            assert np.array_equal(_down_ct(ce, nq - 1), halves[0]) and np.array_equal(_down_ct(co, nq - 1), halves[1]), "inputs unchanged"
    ctx.sync()


@pytest.mark.parametrize("gadget", ["multiP", "singleP", "base2"])
def test_split_merge_random_keys_12_to_11(ctx, gadget):
    np_ = {"multiP": 3, "singleP": 1, "base2": 1}[gadget]
    q, p = _moduli(14, [50] * 6, [55 if gadget != "base2" else 61] * np_)
    _split_merge_case(ctx, 12, q, p, 20 if gadget == "base2" else 0, 8500 + np_ + (10 if gadget == "base2" else 0))


def test_split_merge_random_keys_reference_shape(ctx):
    """10 -> 9 with one 60-bit Q and one 60-bit P, the reference's own test parameters"""
    q, p = _moduli(11, [60], [60])
    _split_merge_case(ctx, 10, q, p, 0, 8520, levels=(0,))


def test_split_merge_c5_moduli(ctx):
    """16 -> 15 with the c5 shape's 25 + 5 moduli (the fused key-switch pipelines at full size), once"""
    q, p = _moduli(17, C5_LOGQ, C5_LOGP)
    _split_merge_case(ctx, 16, q, p, 0, 8530, batches=(1,), levels=(len(q) - 1,))


# ---- 4. the step kernels alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logN", [5, 12])
def test_expand_step(ctx, logN):
    q, _ = _moduli(13, [60, 45])
    N = 1 << logN
    g, o = la.Ring(ctx, N, q), O.Ring(N, q)
    rng = rng_for(8600 + logN)
    xinv = REF.GenXPow2NTT(o, logN, True)
    L = _lib.load()
    level = 1
    for m in (1, 3):
        cin = [_stack(rng, q, N, m) for _ in range(2)]
        tmp = [_stack(rng, q, N, m) for _ in range(2)]
        if m == 3:
            cin[0][1] = np.array([[qi - 1] * N for qi in q], dtype=np.uint64)
            tmp[0][1] = 0
        pin, ptmp = [_up(g, x) for x in cin], [_up(g, x) for x in tmp]
        add = [np.stack([o.binop("Add", cin[c][e], tmp[c][e]) for e in range(m)]) for c in range(2)]
        sub = [np.stack([o.binop("Sub", cin[c][e], tmp[c][e]) for e in range(m)]) for c in range(2)]
        for k in range(logN):
            out = [la.Poly(g, 2, 2 * m) for _ in range(2)]
            _lib.check(L.he_ringpack_expand_step(g.h, level, k, 0, pin[0].h, pin[1].h, ptmp[0].h, ptmp[1].h, out[0].h, out[1].h))
            for c in range(2):
                got = out[c].download()
                assert np.array_equal(got[:m], add[c]), ("sum", logN, k, m, c)
                want = np.stack([o.binop("MulCoeffsMontgomery", sub[c][e], xinv[k]) for e in range(m)])
                assert np.array_equal(got[m:], want), ("difference", logN, k, m, c)
            # sum_only: into a fresh output, and in place (the reference's Add(c0, tmp, c0))
            so = [la.Poly(g, 2, m) for _ in range(2)]
            _lib.check(L.he_ringpack_expand_step(g.h, level, k, 1, pin[0].h, pin[1].h, ptmp[0].h, ptmp[1].h, so[0].h, so[1].h))
            ip = [_up(g, x) for x in cin]
            _lib.check(L.he_ringpack_expand_step(g.h, level, k, 1, ip[0].h, ip[1].h, ptmp[0].h, ptmp[1].h, ip[0].h, ip[1].h))
            for c in range(2):
                assert np.array_equal(so[c].download(), add[c]) and np.array_equal(ip[c].download(), add[c]), ("sum_only", logN, k, m, c)
        assert all(np.array_equal(pin[c].download(), cin[c]) and np.array_equal(ptmp[c].download(), tmp[c]) for c in range(2))
    ctx.sync()


def _pair_list(rng, q, N):
    """pairs of all three kinds: (a, b) as [2][L][N] arrays or None"""
    ct = lambda: np.stack([uniform_poly(rng, q, N) for _ in range(2)])
    pairs = [(ct(), ct()), (ct(), None), (None, ct()), (ct(), ct()), (None, ct())]
    pairs[3][0][0][:] = np.array([[qi - 1] * N for qi in q], dtype=np.uint64)
    kinds = {("both" if a is not None and b is not None else "a" if a is not None else "b") for a, b in pairs}
    assert kinds == {"both", "a", "b"}
    return pairs


@pytest.mark.parametrize("logN", [5, 12])
def test_pack_steps(ctx, logN):
    q, _ = _moduli(13, [60, 45])
    N = 1 << logN
    g, o = la.Ring(ctx, N, q), O.Ring(N, q)
    rng = rng_for(8700 + logN)
    xpow = REF.GenXPow2NTT(o, logN, False)
    L = _lib.load()
    level = 1
    mul = lambda c, x: np.stack([o.binop("MulCoeffsMontgomery", c[i], x) for i in range(2)])
    add = lambda a, b: np.stack([o.binop("Add", a[i], b[i]) for i in range(2)])
    sub = lambda a, b: np.stack([o.binop("Sub", a[i], b[i]) for i in range(2)])
    for k in range(logN):
        pairs = _pair_list(rng, q, N)
        count = len(pairs)
        A = [(_up_ct(g, a) if a is not None else None) for a, _ in pairs]
        B = [(_up_ct(g, b) if b is not None else None) for _, b in pairs]
        nil = [None, None]
        arrs = [R._harr([(x or nil)[c] for x in side]) for side in (A, B) for c in range(2)]
        T = [la.Poly(g, 2, count) for _ in range(2)]
        _lib.check(L.he_ringpack_pack_pre(g.h, level, k, count, *arrs, T[0].h, T[1].h))
        gT = np.stack([t.download() for t in T], axis=1)  # [count][2][L][N]
        wa, wb = [], []
        for z, (a, b) in enumerate(pairs):
            if a is not None and b is not None:
                bx = mul(b, xpow[k])
                assert np.array_equal(gT[z], sub(a, bx)), ("pre both T", logN, k, z)
                wa.append(add(a, bx)); wb.append(b)  # (b is left as it was: the reference discards it)
            elif a is not None:
                assert np.array_equal(gT[z], a), ("pre a T", logN, k, z)
                wa.append(a); wb.append(None)
            else:
                bx = mul(b, xpow[k])
                assert np.array_equal(gT[z], bx), ("pre b T", logN, k, z)
                wa.append(None); wb.append(bx)
        for z in range(count):
            if wa[z] is not None:
                assert np.array_equal(_down_ct(A[z], level)[0], wa[z]), ("pre a", logN, k, z)
            if wb[z] is not None:
                assert np.array_equal(_down_ct(B[z], level)[0], wb[z]), ("pre b", logN, k, z)
        # the automorphism's result stands in T: any words do
        tw = np.stack([np.stack([uniform_poly(rng, q, N) for _ in range(2)]) for _ in range(count)])
        for c in range(2):
            T[c].upload(tw[:, c])
        _lib.check(L.he_ringpack_pack_post(g.h, level, count, *arrs, T[0].h, T[1].h))
        for z in range(count):
            if wa[z] is not None:
                assert np.array_equal(_down_ct(A[z], level)[0], add(wa[z], tw[z])), ("post a", logN, k, z)
                if wb[z] is not None:
                    assert np.array_equal(_down_ct(B[z], level)[0], wb[z]), ("post leaves b of a full pair", logN, k, z)
            else:
                assert np.array_equal(_down_ct(B[z], level)[0], sub(wb[z], tw[z])), ("post b", logN, k, z)
        assert np.array_equal(np.stack([t.download() for t in T], axis=1), tw), "post leaves T"
    ctx.sync()


# ---- 4b. launch profile and accounting ---------------------------------------------------------------------------------------------
def _counted(ctx, call):
    """(alg_bytes, alg_valu) of one call, and nothing else"""
    ctx.alg_bytes(reset=True), ctx.alg_valu(reset=True)
    _lib.check(call())
    return ctx.alg_bytes(reset=True), ctx.alg_valu(reset=True)


def _profiled(ctx, call):
    """{kernel: (launches, algorithmic bytes)} of one call after a warm-up (plans and the arena are built on first use)"""
    _lib.check(call())
    ctx.sync()
    ctx.prof_begin()
    _lib.check(call())
    ctx.sync()
    return {k: (v[0], v[2]) for k, v in ctx.prof_end_bytes().items()}


@pytest.mark.parametrize("batch", [1, 2])
def test_split_and_merge_are_the_key_switch_plus_one_map(ctx, batch):
    """he_ringpack_split / he_ringpack_merge, with and without the odd halves: the launches and counters of the same-degree
    he_apply_evaluation_key at that shape and level (measured here) plus exactly one map launch over both components.  The map
    moves, per limb, N + n words per entry (+ n with the odd halves, and their monomial's n words once per launch); it is charged
    1.5 L limbs of N words per component (2 L with the odd halves, and 0.5 L once per call), and one product per odd word."""
    logN = 12
    N, n = 1 << logN, 1 << (logN - 1)
    q, p = _moduli(14, [50] * 6, [55] * 3)
    rng = rng_for(8800 + batch)
    gQ, gP, gn = la.Ring(ctx, N, q), la.Ring(ctx, N, p), la.Ring(ctx, n, q)
    gev = la.Evaluator(gQ, gP)
    k = _random_key(rng, q, p, N)
    gk = gev.NewEvaluationKey(k.q, k.p)
    nq, level = len(q), len(q) - 2
    L = level + 1
    big = [_up(gQ, _stack(rng, q, N, batch)) for _ in range(4)]
    half = [_up(gn, _stack(rng, q, n, batch)) for _ in range(4)]
    lib = _lib.load()
    calls = {
        "same": lambda: lib.he_apply_evaluation_key(gev.h, level, big[0].h, big[1].h, gk.h, big[2].h, big[3].h),
        ("split", True): lambda: lib.he_ringpack_split(gev.h, level, big[0].h, big[1].h, gk.h, half[0].h, half[1].h, half[2].h, half[3].h),
        ("split", False): lambda: lib.he_ringpack_split(gev.h, level, big[0].h, big[1].h, gk.h, half[0].h, half[1].h, 0, 0),
        ("merge", True): lambda: lib.he_ringpack_merge(gev.h, level, half[0].h, half[1].h, half[2].h, half[3].h, gk.h, big[2].h, big[3].h),
        ("merge", False): lambda: lib.he_ringpack_merge(gev.h, level, half[0].h, half[1].h, 0, 0, gk.h, big[2].h, big[3].h),
    }
    prof = {name: _profiled(ctx, call) for name, call in calls.items()}
    acct = {name: _counted(ctx, call) for name, call in calls.items()}
    print(prof, acct)
    assert "ring_split" not in prof["same"] and "ring_merge" not in prof["same"]
    (s0, s1), sv = acct["same"]
    for name in calls:
        if name == "same":
            continue
        kind, odd = name
        kernel, other = ("ring_split", "ring_merge") if kind == "split" else ("ring_merge", "ring_split")
        got = dict(prof[name])
        moved = float((N + (2 if odd else 1) * n) * L * 2 * batch * 8 + (n * L * 8 if odd else 0))
        assert got.pop(kernel) == (1, moved), (name, prof[name])
        assert other not in got
        assert got == prof["same"], (name, got, prof["same"])
        per_entry, shared = 2 * L * (2.0 if odd else 1.5), (0.5 * L if odd else 0.0)
        want = ((s0 + (per_entry + shared) * batch * N * 8, s1 + (per_entry * batch + shared) * N * 8),
                [sv[0] + (2 * L * n * batch if odd else 0), sv[1], sv[2], sv[3]])
        assert acct[name] == want, (name, acct[name], want)


def test_ring_level_entries_accounting(ctx):
    """the counters of every entry that addresses a ring alone, in closed form (limbs of N words; products)"""
    logN, level, batch = 5, 1, 3
    N, n, L = 1 << logN, 1 << (logN - 1), level + 1
    q, _ = _moduli(13, [60, 45, 55])
    rng = rng_for(8810)
    gN, gn = la.Ring(ctx, N, q), la.Ring(ctx, n, q)
    lib = _lib.load()
    limbs = lambda per_entry, shared, B: (float((per_entry + shared) * B * N * 8), float((per_entry * B + shared) * N * 8))
    muls = lambda x: [float(x), 0.0, 0.0, 0.0]
    pN, pe, po = _up(gN, _stack(rng, q, N, batch)), _up(gn, _stack(rng, q, n, batch)), _up(gn, _stack(rng, q, n, batch))
    # the monomial table: L limbs written
    assert _counted(ctx, lambda: lib.he_ring_xpow2_ntt(gN.h, level, 2, 1, pN.h)) == (limbs(L, 0, batch), muls(0))
    # Split's and Merge's maps: 1.5 L, or 2 L with the odd half, whose monomial is read once per call and costs a product per word
    for call in (lambda odd: lib.he_ring_split_ntt(gN.h, level, pN.h, pe.h, po.h if odd else 0),
                 lambda odd: lib.he_ring_merge_ntt(gN.h, level, pe.h, po.h if odd else 0, pN.h)):
        assert _counted(ctx, lambda: call(True)) == (limbs(2.0 * L, 0.5 * L, batch), muls(L * n * batch))
        assert _counted(ctx, lambda: call(False)) == (limbs(1.5 * L, 0, batch), muls(0))
    # an Expand step over m ciphertexts: in, tmp and the sums (and the differences, a product per word) of both components
    m = batch
    cin, tmp = [_up(gN, _stack(rng, q, N, m)) for _ in range(2)], [_up(gN, _stack(rng, q, N, m)) for _ in range(2)]
    out2, out1 = [la.Poly(gN, len(q), 2 * m) for _ in range(2)], [la.Poly(gN, len(q), m) for _ in range(2)]
    step = lambda so, o: lib.he_ringpack_expand_step(gN.h, level, 1, so, cin[0].h, cin[1].h, tmp[0].h, tmp[1].h, o[0].h, o[1].h)
    assert _counted(ctx, lambda: step(0, out2)) == (limbs(2 * L * 4, 0, m), muls(2 * L * N * m))
    assert _counted(ctx, lambda: step(1, out1)) == (limbs(2 * L * 3, 0, m), muls(0))
    # the Pack steps over pairs of all three kinds: before the automorphism a full pair moves 4 polynomials per component, a pair
    # of a alone 2 and of b alone 3, with a product per word wherever b is present; after it every pair moves 3
    pairs = _pair_list(rng, q, N)
    count = len(pairs)
    both, a_only, b_only = (sum(1 for a, b in pairs if (a is not None, b is not None) == kind) for kind in ((True, True), (True, False), (False, True)))
    A = [(_up_ct(gN, a) if a is not None else None) for a, _ in pairs]
    B = [(_up_ct(gN, b) if b is not None else None) for _, b in pairs]
    nil = [None, None]
    arrs = [R._harr([(x or nil)[c] for x in side]) for side in (A, B) for c in range(2)]
    T = [la.Poly(gN, len(q), count) for _ in range(2)]
    assert _counted(ctx, lambda: lib.he_ringpack_pack_pre(gN.h, level, 1, count, *arrs, T[0].h, T[1].h)) == \
        (limbs(2 * L * (4 * both + 2 * a_only + 3 * b_only), 0, 1), muls(2 * L * N * (both + b_only)))
    assert _counted(ctx, lambda: lib.he_ringpack_pack_post(gN.h, level, count, *arrs, T[0].h, T[1].h)) == (limbs(2 * L * 3 * count, 0, 1), muls(0))
    ctx.sync()


# ---- 5. the mirrors ------------------------------------------------------------------------------------------------------------------
def _random_galois_keys(rng, q, p, N, galels):
    return {int(g): _random_key(rng, q, p, N) for g in galels}


@pytest.mark.parametrize("logN,logGap", [(8, 0), (12, 8)])
def test_expand_mirror(ctx, logN, logGap):
    """logN 8, logGap 0: 256 outputs, both branches of `j + n/gap > 0`; logN 12, logGap 8: sixteen outputs, the batched
    automorphisms run the 4096-row pipeline"""
    q, p = _moduli(logN + 1, [55, 45], [58])
    N = 1 << logN
    rng = rng_for(8800 + logN)
    rings = {logN: (O.Ring(N, q), O.Ring(N, p))}
    ext = {logN: _random_galois_keys(rng, q, p, N, REF.GaloisElementsForExpand(N, logN))}
    ref = REF.RingPackingEvaluator(rings, None, ext, None)
    dev, gr = _device(ctx, rings, None, ext, None)
    assert R.GaloisElementsForExpand(2 * N, logN) == REF.GaloisElementsForExpand(N, logN)
    level = 1
    ct = np.stack([uniform_poly(rng, q, N) for _ in range(2)])
    want = ref.Expand(ct, logGap)
    pct = _up_ct(gr[logN][0], ct)
    stack, indices = dev.Expand(level, pct, logGap)
    assert indices == sorted(want) and len(indices) == N >> logGap
    got = _down_ct(stack, level)
    for e, j in enumerate(indices):
        assert np.array_equal(got[e], want[j]), (logN, logGap, j)
    assert np.array_equal(_down_ct(pct, level)[0], ct), "Expand works on a copy of its input"
    ctx.sync()


@pytest.mark.parametrize("zero_garbage", [True, False])
def test_pack_mirror(ctx, zero_garbage):
    logN = 8
    q, p = _moduli(logN + 1, [55, 45], [58])
    N = 1 << logN
    rng = rng_for(8900 + zero_garbage)
    rings = {logN: (O.Ring(N, q), O.Ring(N, p))}
    rep = {logN: _random_galois_keys(rng, q, p, N, REF.GaloisElementsForPack(N, logN))}
    ref = REF.RingPackingEvaluator(rings, None, None, rep)
    dev, gr = _device(ctx, rings, None, None, rep)
    assert R.GaloisElementsForPack(2 * N, logN, logN) == REF.GaloisElementsForPack(N, logN)
    level = 1
    cts = {i: np.stack([uniform_poly(rng, q, N) for _ in range(2)]) for i in range(0, N, 3)}
    want = ref.Pack(cts, logN, zero_garbage)
    got = dev.Pack(level, {i: _up_ct(gr[logN][0], c) for i, c in cts.items()}, logN, zero_garbage)
    assert np.array_equal(_down_ct(got, level)[0], want)
    with pytest.raises(ValueError):
        dev.Pack(level, {}, logN, True)
    ctx.sync()


LOGN_LARGE, LOGN_SMALL = 10, 8


@pytest.fixture(scope="module")
def real_keys(ctx):
    """the reference's test parameters (ring_packing_test.go): logN 10 -> 8, one 60-bit Q, one 60-bit P, ternary secrets"""
    q, p = _moduli(LOGN_LARGE + 1, [60], [60])
    rng = rng_for(9000)
    rings, sk, rsk, ext, rep = REF.gen_test_keys(rng, LOGN_LARGE, LOGN_SMALL, q, p, extract_at=(LOGN_SMALL,),
                                                 repack_at=(LOGN_SMALL, LOGN_LARGE))
    ref = REF.RingPackingEvaluator(rings, rsk, ext, rep)
    dev, gr = _device(ctx, rings, rsk, ext, rep)
    return dict(rng=rng, rings=rings, sk=sk, ref=ref, dev=dev, gr=gr, N=1 << LOGN_LARGE)


def _map_equal(got, want, level):
    assert sorted(got) == sorted(want)
    for i in want:
        assert np.array_equal(_down_ct(got[i], level)[0], want[i]), i


@pytest.mark.parametrize("extract_naive,repack_naive", [(False, True), (True, False)])
def test_extract_permute_repack_real_keys(ctx, real_keys, extract_naive, repack_naive):
    """Extract[Naive] of idx = {17 i} and of a random half, the permutation x -> x + N/2 and Repack[Naive], each step word for word
    and decrypting within the reference's bounds"""
    S = real_keys
    N, level = S["N"], 0
    rQ, skQ = S["rings"][LOGN_LARGE][0], S["sk"][LOGN_LARGE].Q
    rS, skS = S["rings"][LOGN_SMALL][0], S["sk"][LOGN_SMALL].Q
    pt = REF.gen_plaintext(N)
    ct = REF.encrypt(S["rng"], rQ, skQ, pt)
    gQ = S["gr"][LOGN_LARGE][0]
    # Extract / ExtractNaive with idx = {17 i}
    gap = 17
    idx = [i * gap for i in range(N // gap)]
    want = S["ref"].extract(ct, idx, extract_naive)
    got = S["dev"]._extract(level, _up_ct(gQ, ct), idx, extract_naive)
    _map_equal(got, want, level)
    for i in idx:
        d = REF.decrypt_centered(rS, _down_ct(got[i], level)[0], skS)
        d[0] -= int(pt[i])
        if extract_naive:
            assert np.log2(max(abs(int(d[0])), 1)) <= LOGN_LARGE
        else:
            assert REF.log2_std(d) <= LOGN_LARGE + gap.bit_length() + 1
    # a random half of the coefficients -> permute -> Repack
    idx = sorted(int(x) for x in rng_for(9100).permutation(N)[: N // 2])
    want = S["ref"].extract(ct, idx, extract_naive)
    got = S["dev"]._extract(level, _up_ct(gQ, ct), idx, extract_naive)
    _map_equal(got, want, level)
    permute = lambda x: (x + N // 2) & (N - 1)
    want_ct = S["ref"].repack({permute(i): c for i, c in want.items()}, repack_naive)
    got_ct = S["dev"]._repack(level, {permute(i): c for i, c in got.items()}, repack_naive)
    out = _down_ct(got_ct, level)[0]
    assert np.array_equal(out, want_ct)
    dec = REF.decrypt_centered(rQ, out, skQ)
    for k0 in idx:
        dec[permute(k0)] -= int(pt[k0])
    assert REF.log2_std(dec) <= LOGN_LARGE + 5
    ctx.sync()


def test_repack_gap_three_family_real_keys(ctx, real_keys):
    """ring_packing_test.go:322-383: ciphertext i (i = 0, 3, 6, ...) holds pt * X^-i; Repack returns pt on those coefficients"""
    S = real_keys
    N, level = S["N"], 0
    rQ, skQ = S["rings"][LOGN_LARGE][0], S["sk"][LOGN_LARGE].Q
    pt = REF.gen_plaintext(N)
    cts = {i: REF.encrypt(S["rng"], rQ, skQ, np.concatenate([pt[i:], -pt[:i]])) for i in range(0, N, 3)}
    want = S["ref"].Repack(cts)
    got = S["dev"].Repack(level, {i: _up_ct(S["gr"][LOGN_LARGE][0], c) for i, c in cts.items()})
    out = _down_ct(got, level)[0]
    assert np.array_equal(out, want)
    dec = REF.decrypt_centered(rQ, out, skQ)
    dec[0::3] -= pt[0::3]
    assert REF.log2_std(dec) <= LOGN_LARGE + 5
    ctx.sync()


# ---- 6. one program over all eight entries: the queue, deferred submission, graphs, replay ------------------------------------------
class _Program:
    """operands of one caller and the calls over them; every call writes polynomials nobody else reads, the pack steps work on
    copies made inside the program, so the program gives the same results every time it runs"""

    def __init__(self, S, rng):
        self.S = S
        q, N, n = S["q"], S["N"], S["N"] // 2
        gN, gn = S["gN"], S["gn"]
        nq = len(q)
        self.level = nq - 1
        rnd = lambda g, deg: la.Poly(g, nq).upload(uniform_poly(rng, q, deg))
        new = lambda g, b=1: la.Poly(g, nq, b)
        self.ct = [rnd(gN, N), rnd(gN, N)]
        self.src_a, self.src_b = [rnd(gN, N), rnd(gN, N)], [rnd(gN, N), rnd(gN, N)]
        self.x, self.e, self.o, self.m = new(gN), new(gn), new(gn), new(gN)
        self.even, self.odd, self.out = [new(gn), new(gn)], [new(gn), new(gn)], [new(gN), new(gN)]
        self.exp = [new(gN, 2), new(gN, 2)]
        self.a, self.b, self.t = [new(gN), new(gN)], [new(gN), new(gN)], [new(gN), new(gN)]
        self.results = [self.x, self.e, self.o, self.m] + self.even + self.odd + self.out + self.exp + self.a + self.b + self.t

    def run(self):
        S, lv, L = self.S, self.level, _lib.load()
        gN, dev = S["gN"], S["dev"]
        R.XPow2NTT(gN, lv, 3, True, self.x)
        R.SplitNTT(gN, lv, self.ct[0], self.e, self.o)
        R.MergeNTT(gN, lv, self.e, self.o, self.m)
        dev.Split(lv, self.ct, self.even, self.odd)
        dev.Merge(lv, self.even, self.odd, self.out)
        _lib.check(L.he_ringpack_expand_step(gN.h, lv, 2, 0, self.ct[0].h, self.ct[1].h, self.out[0].h, self.out[1].h,
                                             self.exp[0].h, self.exp[1].h))
        for d, s in zip(self.a + self.b, self.src_a + self.src_b):
            d.CopyLvl(lv, s)
        arrs = [R._harr([self.a[0]]), R._harr([self.a[1]]), R._harr([self.b[0]]), R._harr([self.b[1]])]
        _lib.check(L.he_ringpack_pack_pre(gN.h, lv, 1, 1, *arrs, self.t[0].h, self.t[1].h))
        _lib.check(L.he_ringpack_pack_post(gN.h, lv, 1, *arrs, self.t[0].h, self.t[1].h))

    def get(self):
        return [p.download() for p in self.results]

    def zero(self):
        for p in self.results:
            p.Zero()


@pytest.fixture(scope="module")
def prog_setup(ctx):
    logN = 12
    q, p = _moduli(logN + 1, [55] * 4, [58] * 2)
    N = 1 << logN
    rng = rng_for(9200)
    rings = {logN - 1: (O.Ring(N // 2, q), O.Ring(N // 2, p)), logN: (O.Ring(N, q), O.Ring(N, p))}
    rsk = {(logN, logN - 1): _random_key(rng, q, p, N), (logN - 1, logN): _random_key(rng, q, p, N)}
    dev, gr = _device(ctx, rings, rsk)
    return dict(q=q, N=N, rng=rng, dev=dev, gN=gr[logN][0], gn=gr[logN - 1][0])


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("deferred", [0, 4])
def test_program_through_the_queue(ctx, prog_setup, deferred):
    S = prog_setup
    T = 3
    progs = [_Program(S, rng_for(9300 + t)) for t in range(T)]
    want = []
    for pr in progs:  # alone, with the queue off
        pr.run()
        ctx.sync()
        want.append(pr.get())
        pr.zero()
    assert any(w.any() for w in want[0])
    ctx.SetCoalescing(64, 2000)
    if deferred:
        ctx.SetDeferred(deferred)
    try:
        barrier, errs = threading.Barrier(T), []

        def worker(t):
            try:
                barrier.wait()
                progs[t].run()
            except Exception as e:  # noqa: BLE001
                errs.append(e)
                barrier.abort()

        th = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
        [x.start() for x in th]
        [x.join() for x in th]
        ctx.sync()
        assert not errs, errs
    finally:
        if deferred:
            ctx.SetDeferred(0)
        ctx.SetCoalescing(0, 0)
    for t in range(T):
        assert _same(progs[t].get(), want[t]), t


def test_program_graph_and_replay(ctx, prog_setup):
    S = prog_setup
    pr = _Program(S, rng_for(9400))
    pr.run()  # (plans and the arena are built on first use)
    ctx.sync()
    want = pr.get()
    pr.zero()
    with ctx.capture() as g:
        pr.run()
    for _ in range(2):
        g.launch()
        ctx.sync()
        assert _same(pr.get(), want)
        pr.zero()
    _lib.trace_begin()
    try:
        pr.run()
    finally:
        prog = _lib.trace_end()
    ctx.sync()
    assert _same(pr.get(), want)
    pr.zero()
    ctx.sync()
    _lib.replay(ctx.h, prog, 1, 1, [], [], [])
    ctx.sync()
    assert _same(pr.get(), want)


# ---- 7. rejections leave every operand unchanged --------------------------------------------------------------------------------------
def test_rejections_leave_every_operand_unchanged(ctx, prog_setup):
    S = prog_setup
    q, N, gN, gn, dev = S["q"], S["N"], S["gN"], S["gn"], S["dev"]
    rng = rng_for(9500)
    nq = len(q)
    level = nq - 1
    ev = dev.Evaluators[12]
    k_down, k_up = dev.RingSwitchingKeys[(12, 11)], dev.RingSwitchingKeys[(11, 12)]
    qci, pci = _moduli(14, [55] * 4, [58] * 2)
    cN, cn, cP = la.Ring(ctx, N, qci, conjugate_invariant=True), la.Ring(ctx, N // 2, qci, conjugate_invariant=True), \
        la.Ring(ctx, N, pci, conjugate_invariant=True)
    cev = la.Evaluator(cN, cP)
    okci = _random_key(rng, qci, pci, N)
    kci = cev.NewEvaluationKey(okci.q, okci.p)
    g16, g8k = la.Ring(ctx, 16, q), la.Ring(ctx, N // 4, q)
    # a key with fewer Q limbs than the level asks for
    oks = _random_key(rng, q[:-1], S["dev"].Evaluators[12].ringP.moduli, N)
    k_short = ev.NewEvaluationKey(oks.q, oks.p)
    rnd = lambda g, b=1: la.Poly(g, nq, b).upload(_stack(rng, g.moduli, g.N, b))
    big = [rnd(gN) for _ in range(8)]
    small = [rnd(gn) for _ in range(6)]
    big2, big3 = [rnd(gN, 2) for _ in range(2)], [rnd(gN, 3) for _ in range(2)]
    cbig, csmall = [rnd(cN) for _ in range(4)], [rnd(cn) for _ in range(4)]
    p16, q16 = rnd(g16), rnd(g16)  # a degree-16 input: its halves would be of degree 8, which no ring (logN >= 4) can allocate
    quarter = [rnd(g8k) for _ in range(2)]
    many = [la.Poly(g16, nq, 32768) for _ in range(4)]  # 2 x 32768 entries: one more than a launch's z dimension takes
    allp = big + small + big2 + big3 + cbig + csmall + [p16, q16] + quarter
    before = [p.download() for p in allp]
    L = _lib.load()
    H = R._harr
    h = lambda ps: [p.h for p in ps]
    cases = [
        # conjugate-invariant rings: every entry
        lambda: L.he_ring_xpow2_ntt(cN.h, level, 0, 0, cbig[0].h),
        lambda: L.he_ring_split_ntt(cN.h, level, cbig[0].h, csmall[0].h, csmall[1].h),
        lambda: L.he_ring_merge_ntt(cN.h, level, csmall[0].h, csmall[1].h, cbig[0].h),
        lambda: L.he_ringpack_split(cev.h, level, cbig[0].h, cbig[1].h, kci.h, *h(csmall)),
        lambda: L.he_ringpack_merge(cev.h, level, *h(csmall), kci.h, cbig[0].h, cbig[1].h),
        lambda: L.he_ringpack_expand_step(cN.h, level, 0, 1, *h(cbig), cbig[0].h, cbig[1].h),
        lambda: L.he_ringpack_pack_pre(cN.h, level, 0, 1, H([cbig[0]]), H([cbig[1]]), H([None]), H([None]), cbig[2].h, cbig[3].h),
        lambda: L.he_ringpack_pack_post(cN.h, level, 1, H([cbig[0]]), H([cbig[1]]), H([None]), H([None]), cbig[2].h, cbig[3].h),
        # small degree 8
        lambda: L.he_ring_split_ntt(g16.h, level, p16.h, q16.h, 0),
        lambda: L.he_ring_merge_ntt(g16.h, level, q16.h, 0, p16.h),
        # wrong large degree: the ring / evaluator is not of the large polynomial's degree
        lambda: L.he_ring_split_ntt(gN.h, level, small[0].h, quarter[0].h, quarter[1].h),
        lambda: L.he_ring_merge_ntt(gN.h, level, quarter[0].h, quarter[1].h, small[0].h),
        lambda: L.he_ringpack_split(ev.h, level, small[0].h, small[1].h, k_down.h, quarter[0].h, quarter[1].h, 0, 0),
        lambda: L.he_ringpack_merge(ev.h, level, quarter[0].h, quarter[1].h, 0, 0, k_up.h, small[0].h, small[1].h),
        lambda: L.he_ringpack_split(ev.h, level, big[0].h, big[1].h, k_down.h, big[2].h, big[3].h, 0, 0),  # halves of degree N
        # batch mismatch: the expand step's out is not 2 m (or m in the sum_only form)
        lambda: L.he_ringpack_expand_step(gN.h, level, 0, 0, *h(big[:4]), big[4].h, big[5].h),
        lambda: L.he_ringpack_expand_step(gN.h, level, 0, 0, *h(big[:4]), big3[0].h, big3[1].h),
        lambda: L.he_ringpack_expand_step(gN.h, level, 0, 1, *h(big[:4]), big2[0].h, big2[1].h),
        lambda: L.he_ringpack_split(ev.h, level, big2[0].h, big2[1].h, k_down.h, *h(small[:4])),
        # operand identity
        lambda: L.he_ringpack_split(ev.h, level, big[0].h, big[1].h, k_down.h, small[0].h, small[1].h, small[0].h, small[2].h),  # even0 == odd0
        lambda: L.he_ring_split_ntt(gN.h, level, big[0].h, small[0].h, small[0].h),
        lambda: L.he_ringpack_merge(ev.h, level, *h(small[:4]), k_up.h, big[0].h, big[0].h),
        lambda: L.he_ringpack_expand_step(gN.h, level, 0, 0, *h(big[:4]), big2[0].h, big2[0].h),
        lambda: L.he_ringpack_expand_step(gN.h, level, 0, 1, *h(big[:4]), big[2].h, big[5].h),   # out0 == tmp0
        lambda: L.he_ringpack_expand_step(gN.h, level, 0, 1, *h(big[:4]), big[1].h, big[0].h),   # crossed
        lambda: L.he_ringpack_split(ev.h, level, big[0].h, big[1].h, k_down.h, small[0].h, small[1].h, small[2].h, 0),  # one odd half
        # a handle twice in a pair list
        lambda: L.he_ringpack_pack_pre(gN.h, level, 0, 2, H([big[0], big[2]]), H([big[1], big[3]]), H([None, big[0]]), H([None, big[4]]),
                                       big2[0].h, big2[1].h),
        lambda: L.he_ringpack_pack_pre(gN.h, level, 0, 1, H([big[0]]), H([big[0]]), H([None]), H([None]), big[2].h, big[3].h),
        lambda: L.he_ringpack_pack_post(gN.h, level, 1, H([big[0]]), H([big[1]]), H([None]), H([None]), big[0].h, big[3].h),
        lambda: L.he_ringpack_pack_pre(gN.h, level, 0, 1, H([big[0]]), H([big[1]]), H([None]), H([None]), big[2].h, big[2].h),
        # count = 0, empty pairs, half-given ciphertexts, a batched a, T of the wrong batch, k out of range
        lambda: L.he_ringpack_pack_pre(gN.h, level, 0, 0, H([big[0]]), H([big[1]]), H([None]), H([None]), big[2].h, big[3].h),
        lambda: L.he_ringpack_pack_post(gN.h, level, 0, H([big[0]]), H([big[1]]), H([None]), H([None]), big[2].h, big[3].h),
        lambda: L.he_ringpack_pack_pre(gN.h, level, 0, 1, H([None]), H([None]), H([None]), H([None]), big[2].h, big[3].h),
        lambda: L.he_ringpack_pack_pre(gN.h, level, 0, 1, H([big[0]]), H([None]), H([None]), H([None]), big[2].h, big[3].h),
        lambda: L.he_ringpack_pack_pre(gN.h, level, 0, 1, H([big2[0]]), H([big2[1]]), H([None]), H([None]), big[2].h, big[3].h),
        lambda: L.he_ringpack_pack_pre(gN.h, level, 0, 1, H([big[0]]), H([big[1]]), H([None]), H([None]), big2[0].h, big2[1].h),
        lambda: L.he_ringpack_pack_pre(gN.h, level, 12, 1, H([big[0]]), H([big[1]]), H([None]), H([None]), big[2].h, big[3].h),
        lambda: L.he_ringpack_expand_step(gN.h, level, 12, 1, *h(big[:4]), big[0].h, big[1].h),
        # more entries than one call covers
        lambda: L.he_ringpack_expand_step(g16.h, level, 0, 1, *h(many), many[0].h, many[1].h),
        # level out of range; a key that does not reach the level
        lambda: L.he_ring_split_ntt(gN.h, nq, big[0].h, small[0].h, small[1].h),
        lambda: L.he_ringpack_split(ev.h, level, big[0].h, big[1].h, k_short.h, *h(small[:4])),
        lambda: L.he_ringpack_merge(ev.h, level, *h(small[:4]), k_short.h, big[0].h, big[1].h),
    ]
    for i, c in enumerate(cases):
        assert c() == EINVAL, (i, _lib.load().he_last_error())
    ctx.sync()
    for i, (p, b) in enumerate(zip(allp, before)):
        assert np.array_equal(p.download(), b), i
    # the short key serves the level it has
    dev2 = R.RingPackingEvaluator(dev.Evaluators, {(12, 11): k_short})
    dev2.Split(level - 1, big[:2], small[:2], small[2:4])
    ctx.sync()
