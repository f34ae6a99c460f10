"""The RGSW external product on the device (include/hering_rgsw.h, lattigo_amd.rgsw), word for word against tests/rgsw_ref.py
-- core/rgsw/evaluator.go restated on the oracle -- with uniformly random operands and keys, at the smallest shapes at which each
route and branch can still go wrong."""
import ctypes as C
import gc
import itertools
import threading

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd import _lib
from lattigo_amd import rgsw as G
from oracle import oracle as O
from tests import rgsw_aliasing as RA
from tests import rgsw_ref as R
from tests.gpu_common import ctx  # noqa: F401
from tests.helpers import rng_for, uniform_poly

pytestmark = pytest.mark.gpu

EINVAL = -1
KERNEL = "rgsw_external_product"


@pytest.fixture(autouse=True)
def _no_garbage_left_behind():
    gc.collect()
    yield
    gc.collect()


class Setup:
    """One parameter set on both sides: oracle rings and evaluator, device rings and rgsw.Evaluator."""

    def __init__(self, ctx, logN, q, p, pw2, ci=False):
        self.N, self.q, self.p, self.pw2 = 1 << logN, list(q), list(p), pw2
        self.oQ = O.Ring(self.N, self.q, ci)
        self.oP = O.Ring(self.N, self.p, ci) if self.p else None
        self.oev = O.Evaluator(self.oQ, self.oP)
        self.gQ = la.Ring(ctx, self.N, self.q, conjugate_invariant=ci)
        self.gP = la.Ring(ctx, self.N, self.p, conjugate_invariant=ci) if self.p else None
        self.gev = G.Evaluator(self.gQ, self.gP)
        self.level = len(self.q) - 1

    def rgsw(self, rng):
        """(oracle pair, device rgsw.Ciphertext) with uniformly random words"""
        o = R.uniform_rgsw(rng, self.oQ, self.oP, self.pw2)
        kw = dict(BaseTwoDecomposition=self.pw2, BaseTwoDecompositionVectorSize=o[0].nj) if self.pw2 else {}
        return o, self.gev.NewCiphertext(o[0].q, o[0].p if self.p else None, o[1].q, o[1].p if self.p else None, **kw)

    def cts(self, rng, batch):
        return np.stack([np.stack([uniform_poly(rng, self.q, self.N) for _ in range(2)]) for _ in range(batch)])

    def up(self, ct, nlimbs=None):
        """[B][2][L][N] -> [Poly, Poly]"""
        B, L = ct.shape[0], ct.shape[2]
        out = []
        for k in range(2):
            arr = np.ascontiguousarray(ct[:, k])
            if nlimbs and nlimbs > L:
                arr = np.concatenate([arr, np.full((B, nlimbs - L, self.N), 0x5A5A, dtype=np.uint64)], axis=1)
            out.append(la.Poly(self.gQ, arr.shape[1], B).upload(arr))
        return out

    def down(self, polys):
        return np.stack([p.download()[:, : self.level + 1] for p in polys], axis=1)

    def want(self, ct, orgsw):
        return np.stack([R.external_product(self.oev, ct[b], orgsw) for b in range(ct.shape[0])])

    def new_ct(self, batch):
        return [la.Poly(self.gQ, self.level + 1, batch) for _ in range(2)]


def _moduli(logN, logq, logp=(), ci=False):
    q, p = O.GenModuli(logN + (2 if ci else 1), list(logq), list(logp))
    return list(q), list(p)


def _check(S, seed, batch, inplace=False):
    rng = rng_for(seed)
    orgsw, drgsw = S.rgsw(rng)
    ct = S.cts(rng, batch)
    want = S.want(ct, orgsw)
    op0 = S.up(ct)
    out = op0 if inplace else S.new_ct(batch)
    S.gev.ExternalProduct(op0, drgsw, out)
    got = S.down(out)
    assert np.array_equal(got, want)
    if not inplace:
        assert np.array_equal(S.down(op0), ct), "the inputs were changed"
    return orgsw, drgsw, ct, want


# ---- 1. branch S, the one-launch kernel ------------------------------------------------------------------------------------------
def _q27(logN):
    return O.GenModuli(logN + 1, [27], [])[0][0]


@pytest.mark.parametrize("logN,q", [(9, 0x3001), (10, 0x7FFF801), (11, None)])
def test_32bit_branch_one_launch(ctx, logN, q):
    S = Setup(ctx, logN, [q or _q27(logN)], [], 7)
    orgsw, _, _, _ = _check(S, 8100 + logN, 3)
    assert R.takes_32bit_branch(S.oQ, orgsw) and R.wrap_bound_holds(S.oQ, orgsw)


def test_32bit_branch_wrap_bound_is_refused(ctx):
    logN, N = 10, 1 << 10
    q = (1 << 29) + 1
    while True:  # the largest NTT-friendly prime below 2^29
        q -= 2 * N
        if O.IsPrime(q):
            break
    S = Setup(ctx, logN, [q], [], 4)
    rng = rng_for(8150)
    orgsw, drgsw = S.rgsw(rng)
    assert R.takes_32bit_branch(S.oQ, orgsw) and not R.wrap_bound_holds(S.oQ, orgsw)
    ct = S.cts(rng, 1)
    op0, out = S.up(ct), S.up(ct)
    with pytest.raises(la.HeringError) as e:
        S.gev.ExternalProduct(op0, drgsw, out)
    assert e.value.code == EINVAL and "2^64" in str(e.value)
    assert np.array_equal(S.down(out), ct)


# ---- 2. branch B in one launch, a window wider than its modulus -------------------------------------------------------------------
@pytest.fixture(scope="module")
def b_moduli():
    return _moduli(10, [35, 20], [61])


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("pw2", [7, 13, 0])
def test_bit_windows_with_special_prime(ctx, b_moduli, pw2, inplace):
    q, p = b_moduli
    _check(Setup(ctx, 10, q, p, pw2), 8200 + pw2 + 50 * inplace, 2, inplace)


# ---- 3. branch B where the 32-bit branch does not apply ----------------------------------------------------------------------------
@pytest.mark.parametrize("logq", [(35, 20), (35,)], ids=["two-limbs", "one-35-bit-limb"])
def test_bit_windows_without_special_prime(ctx, logq):
    q, _ = _moduli(10, logq)
    _check(Setup(ctx, 10, q, [], 7), 8300 + len(logq), 2)


# ---- 4. the generic route of branch B (outside the one-launch domain) --------------------------------------------------------------
@pytest.mark.parametrize("logq,logp,pw2", [((35, 20), (61,), 7), ((35, 20), (61,), 13), ((35, 20), (61,), 0), ((35, 20), (), 7), ((35,), (), 7)],
                         ids=["P-pw2-7", "P-pw2-13", "P-all-ones", "no-P", "one-limb"])
def test_bit_windows_generic_route(ctx, logq, logp, pw2):
    q, p = _moduli(13, logq, logp)
    S = Setup(ctx, 13, q, p, pw2)
    _check(S, 8400 + pw2 + len(logq) + 3 * len(logp), 2)
    _check(S, 8450 + pw2 + len(logq) + 3 * len(logp), 1, inplace=True)


# ---- 5. branch M -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logN,logq,logp,batch", [(10, (35, 20), (61, 61), 1), (13, (60, 45, 45, 40), (61, 61), 2)],
                         ids=["rgsw_test.go", "logN13-both-classes"])
def test_multiple_special_primes(ctx, logN, logq, logp, batch):
    q, p = _moduli(logN, logq, logp)
    S = Setup(ctx, logN, q, p, 0)
    _check(S, 8500 + logN, batch)
    _check(S, 8550 + logN, batch, inplace=True)


# ---- 6. a conjugate-invariant ring ------------------------------------------------------------------------------------------------
def test_conjugate_invariant_ring(ctx):
    q, p = _moduli(10, [35, 20], [61], ci=True)
    _check(Setup(ctx, 10, q, p, 7, ci=True), 8600, 2)


# ---- 7. launch counts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["S-9", "S-10", "S-11", "B-7", "B-13", "B-0"])
def test_launch_counts(ctx, b_moduli, shape):
    kind, par = shape.split("-")
    if kind == "S":
        logN = int(par)
        S = Setup(ctx, logN, [{9: 0x3001, 10: 0x7FFF801}.get(logN) or _q27(logN)], [], 7)
    else:
        S = Setup(ctx, 10, b_moduli[0], b_moduli[1], int(par))
    rng = rng_for(8700)
    _, drgsw = S.rgsw(rng)
    op0, out = S.up(S.cts(rng, 2)), S.new_ct(2)
    S.gev.ExternalProduct(op0, drgsw, out)  # (the scratch arena is sized on first use)
    ctx.sync()
    ctx.prof_begin()
    S.gev.ExternalProduct(op0, drgsw, out)
    prof = ctx.prof_end()
    launches = sum(n for n, _ in prof.values())
    print(shape, prof)
    assert KERNEL in prof and prof[KERNEL][0] == 1
    assert launches == 1 if not S.p else launches <= 2


# ---- 8. the select form ------------------------------------------------------------------------------------------------------------
def test_select(ctx, b_moduli):
    q, p = b_moduli
    S = Setup(ctx, 10, q, p, 7)
    rng = rng_for(8800)
    keys = [S.rgsw(rng) for _ in range(3)]
    dset = S.gev.NewKeySet([k[1] for k in keys])
    sel = [2, -1, 0, 0, 1]
    ct = S.cts(rng, 5)
    want = np.stack([ct[b] if s < 0 else R.external_product(S.oev, ct[b], keys[s][0]) for b, s in enumerate(sel)])
    # against per-entry single calls
    for b, s in enumerate(sel):
        if s < 0:
            continue
        one, out1 = S.up(ct[b:b + 1]), S.new_ct(1)
        S.gev.ExternalProduct(one, keys[s][1], out1)
        assert np.array_equal(S.down(out1)[0], want[b])
    op0, out = S.up(ct), S.new_ct(5)
    S.gev.ExternalProductSelect(op0, dset, sel, out)
    assert np.array_equal(S.down(out), want)
    ctx.sync()
    ctx.prof_begin()
    S.gev.ExternalProductSelect(op0, dset, sel, out)
    prof = ctx.prof_end()
    assert prof[KERNEL][0] == 1 and sum(n for n, _ in prof.values()) <= 2, prof  # (the selection's fill is not a profiled kernel)
    assert np.array_equal(S.down(out), want)
    inpl = S.up(ct)
    S.gev.ExternalProductSelect(inpl, dset, sel, inpl)
    assert np.array_equal(S.down(inpl), want)
    # rejections: sel out of range, n_sel != batch; nothing is written
    pre = S.down(out)
    for bad in ([2, -1, 0, 0, 3], [2, -2, 0, 0, 1], [2, -1, 0, 0], [2, -1, 0, 0, 1, 1]):
        with pytest.raises(la.HeringError) as e:
            S.gev.ExternalProductSelect(op0, dset, bad, out)
        assert e.value.code == EINVAL
    assert np.array_equal(S.down(out), pre)


def test_select_outside_the_one_launch_domain(ctx):
    q, p = _moduli(13, [35, 20], [61])
    S = Setup(ctx, 13, q, p, 7)
    rng = rng_for(8850)
    dset = S.gev.NewKeySet([S.rgsw(rng)[1]])
    ct = S.cts(rng, 1)
    op0, out = S.up(ct), S.new_ct(1)
    with pytest.raises(la.HeringError) as e:
        S.gev.ExternalProductSelect(op0, dset, [0], out)
    assert e.value.code == EINVAL


# ---- 9. operand identity and the other rejections ---------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", sorted(RA.ROWS))
def test_operand_identity(ctx, b_moduli, entry):
    row = RA.ROWS[entry]
    q, p = b_moduli
    S = Setup(ctx, 10, q, p, 7)
    rng = rng_for(8900)
    orgsw, drgsw = S.rgsw(rng)
    dset = S.gev.NewKeySet([drgsw])
    L = _lib.load()
    sel = (C.c_int32 * 1)(0)
    names = list(row.params)

    def call(h):
        if entry == "he_rgsw_external_product":
            return L.he_rgsw_external_product(S.gev.h, h["in0"], h["in1"], drgsw.Value[0].h, drgsw.Value[1].h, h["out0"], h["out1"])
        return L.he_rgsw_external_product_select(S.gev.h, h["in0"], h["in1"], dset.h, sel, 1, h["out0"], h["out1"])

    for a, b in itertools.combinations(names, 2):
        words = {n: uniform_poly(rng, S.q, S.N)[None] for n in names}
        polys = {n: la.Poly(S.gQ, S.level + 1, 1).upload(words[n]) for n in names}
        polys[b] = polys[a]
        words[b] = words[a]
        rc = call({n: polys[n].h for n in names})
        got = {n: polys[n].download() for n in names}
        if row.verdict(a, b) == "reject":
            assert rc == EINVAL, (a, b)
            for n in names:
                assert np.array_equal(got[n], words[n]), (a, b, n)
        else:
            assert rc == 0, (a, b, L.he_last_error())
            want = R.external_product(S.oev, np.stack([words["in0"][0], words["in1"][0]]), orgsw)
            assert np.array_equal(got["out0"][0], want[0]) and np.array_equal(got["out1"][0], want[1]), (a, b)


def test_rejections(ctx, b_moduli):
    q, p = b_moduli
    S = Setup(ctx, 10, q, p, 7)
    other = Setup(ctx, 10, q, p, 7)
    rng = rng_for(8950)
    _, drgsw = S.rgsw(rng)
    _, dother = other.rgsw(rng)
    ct = S.cts(rng, 2)
    op0, out = S.up(ct), S.up(ct)
    L = _lib.load()

    def rc(ev, i0, i1, k0, k1, o0, o1):
        return L.he_rgsw_external_product(ev.h, i0.h, i1.h, k0.h, k1.h, o0.h, o1.h)

    assert rc(S.gev, op0[0], op0[1], dother.Value[0], dother.Value[1], out[0], out[1]) == EINVAL  # keys of another evaluator
    assert rc(S.gev, op0[0], op0[1], drgsw.Value[0], dother.Value[1], out[0], out[1]) == EINVAL
    # mismatched key shapes on one evaluator
    o13 = R.uniform_rgsw(rng, S.oQ, S.oP, 13)
    k13 = S.gev.NewEvaluationKey(o13[1].q, o13[1].p, 13, o13[1].nj)
    assert rc(S.gev, op0[0], op0[1], drgsw.Value[0], k13, out[0], out[1]) == EINVAL
    short = la.Poly(S.gQ, 1, 2)
    assert rc(S.gev, short, op0[1], drgsw.Value[0], drgsw.Value[1], out[0], out[1]) == EINVAL      # too few limbs
    assert rc(S.gev, op0[0], op0[1], drgsw.Value[0], drgsw.Value[1], out[0], short) == EINVAL
    one = la.Poly(S.gQ, 2, 1)
    assert rc(S.gev, op0[0], op0[1], drgsw.Value[0], drgsw.Value[1], out[0], one) == EINVAL        # batch mismatch
    assert rc(S.gev, one, op0[1], drgsw.Value[0], drgsw.Value[1], out[0], out[1]) == EINVAL
    assert np.array_equal(S.down(out), ct) and np.array_equal(S.down(op0), ct)


def test_limbs_above_the_level_keep_their_words(ctx, b_moduli):
    q, p = b_moduli
    S = Setup(ctx, 10, q, p, 7)
    rng = rng_for(8960)
    orgsw, drgsw = S.rgsw(rng)
    ct = S.cts(rng, 2)
    # polynomials of three limbs on a ring whose keys have two: limb 2 of the outputs is not touched
    g3 = la.Ring(ctx, S.N, S.q + [_moduli(10, [36])[0][0]])
    fill = np.full((2, 1, S.N), 0x77, dtype=np.uint64)
    op0 = [la.Poly(g3, 3, 2).upload(np.concatenate([ct[:, k], fill], axis=1)) for k in range(2)]
    out = [la.Poly(g3, 3, 2).upload(np.concatenate([ct[:, k], fill + 1], axis=1)) for k in range(2)]
    S.gev.ExternalProduct(op0, drgsw, out)
    for k in range(2):
        got = out[k].download()
        assert np.array_equal(got[:, :2], S.want(ct, orgsw)[:, k]) and np.array_equal(got[:, 2:], fill + 1)


# ---- 10. the submission queue ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deferred", [0, 8], ids=["coalescing", "deferred"])
def test_eight_threads_through_the_queue(ctx, deferred):
    S = Setup(ctx, 10, [0x7FFF801], [], 7)
    rng = rng_for(9000 + deferred)
    T = 8
    keys = [S.rgsw(rng)[1] for _ in range(2)]
    cts = [S.cts(rng, 1) for _ in range(T)]
    ops = [S.up(c) for c in cts]
    outs = [S.new_ct(1) for _ in range(T)]
    want = []
    for t in range(T):  # direct calls, the queue off: a product, then a second one in place with the other key
        S.gev.ExternalProduct(ops[t], keys[t % 2], outs[t])
        S.gev.ExternalProduct(outs[t], keys[1 - t % 2], outs[t])
        want.append(S.down(outs[t]))
        [o.Zero() for o in outs[t]]
    ctx.sync()
    ctx.SetCoalescing(64, 2000)
    if deferred:
        ctx.SetDeferred(deferred)
    try:
        barrier, errs = threading.Barrier(T), []

        def worker(t):
            try:
                barrier.wait()
                S.gev.ExternalProduct(ops[t], keys[t % 2], outs[t])
                S.gev.ExternalProduct(outs[t], keys[1 - t % 2], outs[t])
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
        assert np.array_equal(S.down(outs[t]), want[t]), t


# ---- 11. graph capture -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["one-launch", "generic"])
def test_graph_of_four_chained_products(ctx, b_moduli, fused):
    if fused:
        S = Setup(ctx, 10, b_moduli[0], b_moduli[1], 7)
    else:
        q, p = _moduli(13, [35, 20], [61])
        S = Setup(ctx, 13, q, p, 7)
    rng = rng_for(9100 + fused)
    keys = [S.rgsw(rng)[1] for _ in range(4)]
    ct = S.cts(rng, 2)
    acc = S.up(ct)
    for k in keys:  # the eager chain (also sizes the scratch arena)
        S.gev.ExternalProduct(acc, k, acc)
    ctx.sync()
    want = S.down(acc)
    assert not np.array_equal(want, ct)
    start = S.up(ct)
    [a.CopyLvl(S.level, s) for a, s in zip(acc, start)]
    ctx.sync()
    with ctx.capture() as g:
        for k in keys:
            S.gev.ExternalProduct(acc, k, acc)
    for _ in range(2):
        [a.CopyLvl(S.level, s) for a, s in zip(acc, start)]
        g.launch()
        ctx.sync()
        assert np.array_equal(S.down(acc), want)
    g.close()


def test_select_in_a_graph_freezes_the_selection(ctx, b_moduli):
    S = Setup(ctx, 10, b_moduli[0], b_moduli[1], 7)
    rng = rng_for(9150)
    keys = [S.rgsw(rng) for _ in range(2)]
    dset = S.gev.NewKeySet([k[1] for k in keys])
    ct = S.cts(rng, 3)
    sel = np.array([1, -1, 0], dtype=np.int32)
    want = np.stack([ct[b] if s < 0 else R.external_product(S.oev, ct[b], keys[s][0]) for b, s in enumerate(sel)])
    op0, out = S.up(ct), S.new_ct(3)
    S.gev.ExternalProductSelect(op0, dset, sel, out)
    ctx.sync()
    [o.Zero() for o in out]
    with ctx.capture() as g:
        S.gev.ExternalProductSelect(op0, dset, sel, out)
    sel[:] = [0, 0, 0]  # the caller's array is not read again
    g.launch()
    ctx.sync()
    assert np.array_equal(S.down(out), want)
    g.close()


# ---- 12. the trace recorder and the replayer know the two product entries -----------------------------------------------------------
def test_trace_and_replay(ctx, b_moduli):
    S = Setup(ctx, 10, b_moduli[0], b_moduli[1], 7)
    rng = rng_for(9200)
    orgsw, drgsw = S.rgsw(rng)
    dset = S.gev.NewKeySet([drgsw])
    ct = S.cts(rng, 2)
    want = S.want(ct, orgsw)
    op0, out, out2 = S.up(ct), S.new_ct(2), S.new_ct(2)
    _lib.trace_begin()
    try:
        S.gev.ExternalProduct(op0, drgsw, out)
        S.gev.ExternalProductSelect(op0, dset, [0, -1], out2)
    finally:
        prog = _lib.trace_end()
    ctx.sync()
    [o.Zero() for o in out + out2]
    ctx.sync()
    _lib.replay(ctx.h, prog, 1, 1, [], [], [])
    ctx.sync()
    assert np.array_equal(S.down(out), want)
    got2 = S.down(out2)
    assert np.array_equal(got2[0], want[0]) and np.array_equal(got2[1], ct[1])


# ---- 13. the element-wise helpers on the keys' device words (core/rgsw/evaluator.go:283-356) ---------------------------------------
def _key_words(k):
    """an oracle key as the device stores it: [beta][2][nQk + nPk][N]"""
    return np.concatenate([k.q, k.p], axis=2)


def _same_keys(dev: G.Ciphertext, ora):
    return all(np.array_equal(dev.Value[k].download(), _key_words(ora[k])) for k in range(2))


@pytest.mark.parametrize("logq,logp,pw2", [((35, 20), (61,), 7), ((35, 20), (), 7), ((35, 20), (61, 61), 0), ((35, 20), (61,), 0)],
                         ids=["P-pw2-7", "no-P", "multiple-P", "P-all-ones"])
def test_key_helpers(ctx, logq, logp, pw2):
    q, p = _moduli(10, logq, logp)
    S = Setup(ctx, 10, q, p, pw2)
    rng = rng_for(9300 + pw2 + len(logp))
    oA, dA = S.rgsw(rng)
    oB, dB = S.rgsw(rng)
    oC, dC = S.rgsw(rng)
    # AddLazy of a ciphertext, then Reduce in place and out of place
    G.AddLazy(dA, None, dB)
    oB = R.add_lazy_ciphertext(S.oQ, S.oP, oA, oB)
    assert _same_keys(dB, oB) and _same_keys(dA, oA)
    G.Reduce(dB, None, dC)
    oC = R.reduce(S.oQ, S.oP, oB, oC)
    assert _same_keys(dC, oC) and _same_keys(dB, oB)
    G.Reduce(dB, None, dB)
    assert _same_keys(dB, oC)
    oB = oC
    # the monomial X^alpha - 1 over every (digit, component, limb) row: positive, negative and the largest exponents
    for alpha in (1, -3, S.N - 1, -(S.N - 1)):
        xQ = R.xpow_alpha_minus_one(S.oQ, alpha)
        xP = R.xpow_alpha_minus_one(S.oP, alpha) if S.p else None
        dx = (la.Poly(S.gQ, len(q), 1).upload(xQ[None]), la.Poly(S.gP, len(p), 1).upload(xP[None]) if S.p else None)
        G.MulByXPowAlphaMinusOneLazy(dA, dx, None, dC)
        oC = R.mul_by_xpow_alpha_minus_one_lazy(S.oQ, S.oP, oA, xQ, xP, oC)
        assert _same_keys(dC, oC), alpha
        G.MulByXPowAlphaMinusOneThenAddLazy(dA, dx, None, dB)
        oB = R.mul_by_xpow_alpha_minus_one_lazy(S.oQ, S.oP, oA, xQ, xP, oB, then_add=True)
        assert _same_keys(dB, oB), alpha
    assert _same_keys(dA, oA)
    # in place: A = A (X^alpha - 1), reduced, then used: the product with the new key is the oracle's
    G.MulByXPowAlphaMinusOneLazy(dA, dx, None, dA)
    G.Reduce(dA, None, dA)
    oA = R.reduce(S.oQ, S.oP, R.mul_by_xpow_alpha_minus_one_lazy(S.oQ, S.oP, oA, xQ, xP, oA), oA)
    assert _same_keys(dA, oA)
    ct = S.cts(rng, 1)
    op0, out = S.up(ct), S.new_ct(1)
    S.gev.ExternalProduct(op0, dA, out)
    assert np.array_equal(S.down(out), S.want(ct, oA))
    # AddLazy of a plaintext: one polynomial per window, onto component 0 of the first and component 1 of the second key
    windows = max(oA[0].nj[: len(q)]) if pw2 else 1
    pt = np.stack([uniform_poly(rng, q, S.N) for _ in range(windows)])
    G.AddLazy(G.Plaintext(la.Poly(S.gQ, len(q), windows).upload(pt)), None, dA)
    oA = R.add_lazy_plaintext(S.oQ, S.oP, pt, oA)
    assert _same_keys(dA, oA)


def test_key_helper_rejections(ctx, b_moduli):
    q, p = b_moduli
    S7, S13 = Setup(ctx, 10, q, p, 7), Setup(ctx, 10, q, p, 13)
    rng = rng_for(9350)
    o7, d7 = S7.rgsw(rng)
    _, d13 = S13.rgsw(rng)
    L = _lib.load()
    assert L.he_rgsw_key_op(G.ADD_LAZY, d7.Value[0].h, 0, 0, d13.Value[0].h) == EINVAL    # shapes, evaluators
    assert L.he_rgsw_key_op(7, d7.Value[0].h, 0, 0, d7.Value[1].h) == EINVAL              # unknown operation
    assert L.he_rgsw_key_op(G.MUL_LAZY, d7.Value[0].h, 0, 0, d7.Value[1].h) < 0           # powXMinusOne missing
    short = la.Poly(S7.gQ, 1, 1)
    assert L.he_rgsw_key_add_plaintext_lazy(short.h, d7.Value[0].h, d7.Value[1].h) == EINVAL
    assert L.he_rgsw_key_add_plaintext_lazy(la.Poly(S7.gQ, 2, 5).h, d7.Value[0].h, d7.Value[0].h) == EINVAL
    assert _same_keys(d7, o7)
