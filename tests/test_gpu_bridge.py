"""The CKKS DomainSwitcher on the device (include/hering_bridge.h), word for word against the reference's own sequences restated
in tests/bridge_ref.py: FoldStandardToConjugateInvariant / UnfoldConjugateInvariantToStandard (ring/conjugate_invariant.go:3-44)
and ComplexToReal / RealToComplex (schemes/ckks/bridge.go:57-144)."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd import _lib
from lattigo_amd import bridge as LB
from oracle import oracle as O
from tests import bridge_ref as B
from tests.gpu_common import ctx  # noqa: F401
from tests.helpers import rng_for, uniform_poly
from tests.rlwe_fixtures import SecretKey

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C5_LOGQ = [60] + [40] * 9 + [39] * 3 + [60] * 8 + [56] * 4  # the c5 shape: 25 Q moduli, 5 P moduli
C5_LOGP = [61] * 5
EINVAL, EHANDLE = -1, -2


def _moduli(log_nth, nq, np_=0, bits_q=55, bits_p=61):
    q, p = O.GenModuli(log_nth, [bits_q] * nq, [bits_p] * np_)
    return list(q), list(p)


def _rand(rng, q, N, batch):
    return np.stack([uniform_poly(rng, q, N) for _ in range(batch)])


# ---- ring-level maps ------------------------------------------------------------------------------------------------------------
MAP_Q = [int(x) for x in O.GenModuli(17, [45, 58, 61, 55], [])[0]]  # = 1 mod 2^17: both ring types up to a standard degree of 2^16


def _map_inputs(rng, q, N, batch):
    """[(name, [batch, limbs, N] words)]: random in [0, q); every word q - 1; mirrored pairs (j, N-1-j) summing to exactly q - 1, q
    and q + 1 (either side of the fold's conditional subtraction)"""
    qi = np.array(q, dtype=np.uint64)[None, :, None]
    out = [("random", _rand(rng, q, N, batch)), ("q-1", np.broadcast_to(qi - np.uint64(1), (batch, len(q), N)).copy())]
    for name, d in (("sum q-1", 1), ("sum q", 0), ("sum q+1", -1)):
        a = _rand(rng, q, N, batch)
        lo = a[:, :, : N // 2]
        lo = np.where(lo < 2, lo + np.uint64(2), lo)  # (keeps the partner below q for every target)
        a[:, :, : N // 2] = lo
        a[:, :, N // 2:] = ((qi - np.uint64(d)) - lo)[:, :, ::-1] if d >= 0 else ((qi + np.uint64(1)) - lo)[:, :, ::-1]
        out.append((name, a))
    return out


def _lazy_inputs(rng, q, N, batch):
    """the fold alone: words in [q, 2^64), and pairs whose 64-bit sum wraps"""
    a = rng.integers(0, 1 << 64, size=(batch, len(q), N), dtype=np.uint64)
    qi = np.array(q, dtype=np.uint64)[None, :, None]
    return np.where(a < qi, a + qi, a)


def _check_maps(ctx, n, batch, level, rng, poison=False):
    N, q = 2 * n, MAP_Q
    gstd, gci = la.Ring(ctx, N, q), la.Ring(ctx, n, q, conjugate_invariant=True)
    L = _lib.load()
    ql = q[: level + 1]
    new = lambda ring, pre: (la.Poly(ring, len(q), batch, zero=False) if poison else la.Poly(ring, len(q), batch).upload(pre))
    for name, x in _map_inputs(rng, q, N, batch) + [("lazy", _lazy_inputs(rng, q, N, batch))]:
        pre = _rand(rng, q, n, batch)
        out = new(gci, pre)
        pin = la.Poly(gstd, len(q), batch).upload(x)
        # the moduli may come from a ring of either type and of either degree
        ring = (gci, gstd)[(n + batch + level) % 2]
        if level == len(q) - 1:
            ring.FoldStandardToConjugateInvariant(pin, out)
        else:
            _lib.check(L.he_fold_standard_to_conjugate_invariant(ring.h, level, pin.h, out.h))
        got = out.download()
        for b in range(batch):
            assert np.array_equal(got[b, : level + 1], B.fold(x[b, : level + 1], ql)), ("fold", name, n, batch, level, b)
        if not poison:
            assert np.array_equal(got[:, level + 1:], pre[:, level + 1:]), "limbs above level unchanged"
        assert np.array_equal(pin.download(), x), "input unchanged"
    for name, x in _map_inputs(rng, q, n, batch):
        pre = _rand(rng, q, N, batch)
        out = new(gstd, pre)
        pin = la.Poly(gci, len(q), batch).upload(x)
        if level == len(q) - 1:
            gstd.UnfoldConjugateInvariantToStandard(pin, out)
        else:
            _lib.check(L.he_unfold_conjugate_invariant_to_standard(level, pin.h, out.h))
        got = out.download()
        assert np.array_equal(got[:, : level + 1], B.unfold(x[:, : level + 1])), ("unfold", name, n, batch, level)
        if not poison:
            assert np.array_equal(got[:, level + 1:], pre[:, level + 1:]), "limbs above level unchanged"
        assert np.array_equal(pin.download(), x), "input unchanged"
    ctx.sync()


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n", [16, 512, 1024, 1 << 15])
def test_ring_level_maps(ctx, n, batch):
    """n = 16: a partial workgroup, the mirrored pair next to the forward pair; 512: exactly one workgroup in x; 1 and 3 limbs of
    a handle of 4 (level 0 and 2: 45-bit alone, then 45, 58 and 61 bits)"""
    rng = rng_for(8200 + n + batch)
    for level in (0, 2):
        _check_maps(ctx, n, batch, level, rng)


def poison_case():
    """run by test_every_output_word_is_written in a process of its own with HERING_POISON=1: outputs are scratch polynomials"""
    c = la.Context(0)
    rng = rng_for(8290)
    for n, batch in ((16, 3), (1024, 1)):
        _check_maps(c, n, batch, 3, rng, poison=True)
    c.sync()


def test_every_output_word_is_written(ctx):
    env = dict(os.environ, HERING_POISON="1")
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_bridge import poison_case; poison_case()"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- ComplexToReal / RealToComplex with random key words -----------------------------------------------------------------------
def _random_key(rng, q, p, N, pw2=0):
    if pw2:
        nj = [(int(x).bit_length() + pw2 - 1) // pw2 for x in q]
        D = sum(nj)
    else:
        nj, D = None, O.BaseRNSDecompositionVectorSize(len(q) - 1, len(p) - 1)
    kq = np.stack([np.stack([uniform_poly(rng, q, N) for _ in range(2)]) for _ in range(D)])
    kp = np.stack([np.stack([uniform_poly(rng, p, N) for _ in range(2)]) for _ in range(D)])
    return kq, kp, nj


class _Setup:
    """rings, evaluator and one random key on both sides"""

    def __init__(self, ctx, logN, q, p, pw2, seed):
        self.N, self.n, self.q, self.nq = 1 << logN, 1 << (logN - 1), q, len(q)
        self.rng = rng_for(seed)
        self.gQ, self.gP = la.Ring(ctx, self.N, q), la.Ring(ctx, self.N, p)
        self.gci = la.Ring(ctx, self.n, q, conjugate_invariant=True)
        self.oQ, self.oP = O.Ring(self.N, q), O.Ring(self.N, p)
        self.gev, self.oev = la.Evaluator(self.gQ, self.gP), O.Evaluator(self.oQ, self.oP)
        kq, kp, nj = _random_key(self.rng, q, p, self.N, pw2)
        self.gk = self.gev.NewEvaluationKey(kq, kp, pw2, nj) if pw2 else self.gev.NewEvaluationKey(kq, kp)
        self.ok = O.EvaluationKey(kq, kp, pw2=pw2, nj=nj) if pw2 else O.EvaluationKey(kq, kp)
        self.sw = LB.DomainSwitcher(self.gev, self.gk, self.gk)

    def std(self, x=None, batch=1, limbs=None):
        p = la.Poly(self.gQ, limbs or self.nq, batch)
        return p if x is None else p.upload(x)

    def ci(self, x=None, batch=1, limbs=None):
        p = la.Poly(self.gci, limbs or self.nq, batch)
        return p if x is None else p.upload(x)


def _bridge_case(ctx, logN, q, p, pw2, seed, batches=(1, 2)):
    S = _Setup(ctx, logN, q, p, pw2, seed)
    rng, nq = S.rng, S.nq
    for level in (nq - 1, nq - 2):
        for batch in batches:
            big = [_rand(rng, q, S.N, batch) for _ in range(2)]
            small = [_rand(rng, q, S.n, batch) for _ in range(2)]
            # at the top level through the mirror (level = min of the two), one below through polynomials of one limb fewer
            limbs = level + 1
            i0, i1 = S.std(big[0][:, :limbs], batch, limbs), S.std(big[1][:, :limbs], batch, limbs)
            o = [S.ci(None, batch), S.ci(None, batch)]
            S.sw.ComplexToReal([i0, i1], o)
            got = [x.download() for x in o]
            for b in range(batch):
                want = B.complex_to_real(S.oev, S.oQ, level, [big[0][b], big[1][b]], S.ok)
                for k in range(2):
                    assert np.array_equal(got[k][b, : level + 1], want[k]), ("ComplexToReal", level, batch, b, k)
            assert np.array_equal(i0.download(), big[0][:, :limbs]) and np.array_equal(i1.download(), big[1][:, :limbs]), "inputs unchanged"
            i0, i1 = S.ci(small[0], batch), S.ci(small[1], batch)
            o = [S.std(None, batch, limbs), S.std(None, batch, limbs)]
            S.sw.RealToComplex([i0, i1], o)
            got = [x.download() for x in o]
            for b in range(batch):
                want = B.real_to_complex(S.oev, S.oQ, level, [small[0][b], small[1][b]], S.ok)
                for k in range(2):
                    assert np.array_equal(got[k][b], want[k]), ("RealToComplex", level, batch, b, k)
            assert np.array_equal(i0.download(), small[0]) and np.array_equal(i1.download(), small[1]), "inputs unchanged"
    # in0 == in1 is accepted
    x = _rand(rng, q, S.N, 1)
    i0, o = S.std(x), [S.ci(), S.ci()]
    S.sw.ComplexToReal([i0, i0], o)
    want = B.complex_to_real(S.oev, S.oQ, nq - 1, [x[0], x[0]], S.ok)
    assert all(np.array_equal(o[k].get(), want[k]) for k in range(2))
    ctx.sync()


@pytest.mark.parametrize("gadget", ["multiP", "singleP", "base2"])
def test_bridge_random_keys_12_to_11(ctx, gadget):
    np_ = {"multiP": 3, "singleP": 1, "base2": 1}[gadget]
    q, p = _moduli(14, 6, np_, bits_q=50, bits_p=55 if gadget != "base2" else 61)
    _bridge_case(ctx, 12, q, p, 13 if gadget == "base2" else 0, 8300 + np_ + (10 if gadget == "base2" else 0))


def test_bridge_random_keys_13_to_12(ctx):
    q, p = _moduli(15, 6, 3, bits_q=50, bits_p=55)
    _bridge_case(ctx, 13, q, p, 0, 8320)


def test_bridge_c5_moduli(ctx):
    """16 <-> 15 with the c5 shape's 25 + 5 moduli (the fused key-switch pipelines at full size), batch 1"""
    q, p = O.GenModuli(17, C5_LOGQ, C5_LOGP)
    _bridge_case(ctx, 16, list(q), list(p), 0, 8340, batches=(1,))


def test_bridge_real_keys_round_trip(ctx):
    """the keys of tests/test_bridge_host.py through the device: RealToComplex and ComplexToReal give the reference's words, and
    the round trip decrypts under skCI to 2 m within 2 (EBOUND + KS) + 2 KS (the bounds derived there: the first key switch's
    error is folded, two coefficients per output, and the second adds its own folded error)"""
    logN = 10
    N, n = 1 << logN, 1 << (logN - 1)
    q, p = _moduli(logN + 1, 3, 2)
    rng = rng_for(8400)
    oQ, oP, ciQ = O.Ring(N, q), O.Ring(N, p), O.Ring(n, q, True)
    oev = O.Evaluator(oQ, oP)
    sk_std = SecretKey(rng, oQ, oP)
    sk_ci, _, k_c2r, k_r2c = B.gen_ring_swap_keys(rng, oQ, oP, sk_std, rng.integers(-1, 2, size=n))
    gQ, gP, gci = la.Ring(ctx, N, q), la.Ring(ctx, N, p), la.Ring(ctx, n, q, conjugate_invariant=True)
    gev = la.Evaluator(gQ, gP)
    sw = LB.DomainSwitcher(gev, gev.NewEvaluationKey(k_c2r.q, k_c2r.p), gev.NewEvaluationKey(k_r2c.q, k_r2c.p))
    level = len(q) - 1
    m = rng.integers(-(1 << 30), 1 << 30, size=n)
    ct = B.encrypt(rng, ciQ, sk_ci.Q, m)
    pin = [la.Poly(gci, len(q)).upload(ct[k]) for k in range(2)]
    up, back = [la.Poly(gQ, len(q)) for _ in range(2)], [la.Poly(gci, len(q)) for _ in range(2)]
    sw.RealToComplex(pin, up)
    sw.ComplexToReal(up, back)
    want_up = B.real_to_complex(oev, oQ, level, ct, k_r2c)
    want_back = B.complex_to_real(oev, oQ, level, want_up, k_c2r)
    got_up, got_back = np.stack([x.get() for x in up]), np.stack([x.get() for x in back])
    assert np.array_equal(got_up, want_up) and np.array_equal(got_back, want_back)
    KS = B.key_switch_noise_bound(N, q, p)
    e = max(abs(int(g) - 2 * int(w)) for g, w in zip(B.centred_phase(ciQ, got_back, sk_ci.Q), m))
    assert e <= 2 * (B.EBOUND + KS) + 2 * KS, e
    # without a key the mirror reports the reference's error
    with pytest.raises(la.HeringError, match="no realToComplexEvk provided"):
        LB.DomainSwitcher(gev).RealToComplex(pin, up)


# ---- launch profile ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 2])
def test_launch_profile_is_the_key_switch_plus_one_map(ctx, batch):
    """each call is the same-degree he_apply_evaluation_key's launches at that shape (measured here) plus exactly one map launch
    over both components, charged 1.5 N words per limb and entry"""
    q, p = _moduli(14, 6, 3, bits_q=50, bits_p=55)
    S = _Setup(ctx, 12, q, p, 0, 8500 + batch)
    level = S.nq - 2
    big = [S.std(_rand(S.rng, q, S.N, batch), batch) for _ in range(4)]
    small = [S.ci(_rand(S.rng, q, S.n, batch), batch) for _ in range(4)]
    L = _lib.load()
    calls = {
        "same": lambda: L.he_apply_evaluation_key(S.gev.h, level, big[0].h, big[1].h, S.gk.h, big[2].h, big[3].h),
        "c2r": lambda: L.he_complex_to_real(S.gev.h, level, big[0].h, big[1].h, S.gk.h, small[2].h, small[3].h),
        "r2c": lambda: L.he_real_to_complex(S.gev.h, level, small[0].h, small[1].h, S.gk.h, big[2].h, big[3].h),
    }
    prof = {}
    for name, call in calls.items():
        _lib.check(call())  # (plans and the arena are built on first use)
        ctx.sync()
        ctx.prof_begin()
        _lib.check(call())
        ctx.sync()
        prof[name] = {k: (v[0], v[2]) for k, v in ctx.prof_end_bytes().items()}
    print(prof)
    want_bytes = 1.5 * S.N * (level + 1) * 2 * batch * 8
    for name, kernel, other in (("c2r", "ci_bridge_fold", "ci_bridge_unfold"), ("r2c", "ci_bridge_unfold", "ci_bridge_fold")):
        got = dict(prof[name])
        assert got.pop(kernel) == (1, want_bytes), (name, prof[name])
        assert other not in got
        assert got == prof["same"], (name, got, prof["same"])
    assert "ci_bridge_fold" not in prof["same"] and "ci_bridge_unfold" not in prof["same"]
    # the counters: those of the same-degree key switch plus the map's 1.5 L limbs per component, and no product of its own
    acct = {}
    for name, call in calls.items():
        ctx.alg_bytes(reset=True), ctx.alg_valu(reset=True)
        _lib.check(call())
        acct[name] = (ctx.alg_bytes(reset=True), ctx.alg_valu(reset=True))
    print(acct)
    (s0, s1), sv = acct["same"]
    for name in ("c2r", "r2c"):
        assert acct[name] == ((s0 + want_bytes, s1 + want_bytes), sv), (name, acct[name], acct["same"])


@pytest.mark.parametrize("batch", [1, 3])
def test_ring_level_maps_accounting(ctx, batch):
    """the fold and the unfold alone charge 1.5 L limbs of 2 n words per entry and no arithmetic"""
    n, level = 64, 2
    q = MAP_Q
    rng = rng_for(8550 + batch)
    gstd, gci = la.Ring(ctx, 2 * n, q), la.Ring(ctx, n, q, conjugate_invariant=True)
    pstd, pci = la.Poly(gstd, len(q), batch).upload(_rand(rng, q, 2 * n, batch)), la.Poly(gci, len(q), batch).upload(_rand(rng, q, n, batch))
    L = _lib.load()
    want = float(1.5 * (level + 1) * batch * 2 * n * 8)
    for call in (lambda: L.he_fold_standard_to_conjugate_invariant(gstd.h, level, pstd.h, pci.h),
                 lambda: L.he_unfold_conjugate_invariant_to_standard(level, pci.h, pstd.h)):
        ctx.alg_bytes(reset=True), ctx.alg_valu(reset=True)
        _lib.check(call())
        assert (ctx.alg_bytes(reset=True), ctx.alg_valu(reset=True)) == ((want, want), [0.0] * 4)
    ctx.sync()


# ---- the submission queue, graphs and replay -------------------------------------------------------------------------------------
def _queue_setup(ctx, seed, log_nth=13):
    q, p = _moduli(log_nth, 5, 2)
    return _Setup(ctx, 12, q, p, 0, seed)


@pytest.mark.parametrize("deferred", [0, 4])
def test_queue_coalesced_and_deferred(ctx, deferred):
    """8 threads on their own batch-1 handles, each direction in turn; bit-identical to the direct calls"""
    S = _queue_setup(ctx, 8600 + deferred)
    T, REP = 8, 3
    for name, (mk_in, mk_out, n_in, call) in {"c2r": (S.std, S.ci, S.N, S.sw.ComplexToReal), "r2c": (S.ci, S.std, S.n, S.sw.RealToComplex)}.items():
        data = [[uniform_poly(S.rng, S.q, n_in) for _ in range(2)] for _ in range(T)]
        want = []
        for t in range(T):
            outs = [mk_out(), mk_out()]
            call([mk_in(x) for x in data[t]], outs)
            want.append([o.get() for o in outs])
        ctx.sync()
        ins = [[mk_in(x) for x in data[t]] for t in range(T)]
        outs = [[mk_out(), mk_out()] for _ in range(T)]
        ctx.SetCoalescing(64, 2000)
        if deferred:
            ctx.SetDeferred(deferred)
        try:
            s0 = ctx.CoalescingStats()
            barrier, errs = threading.Barrier(T), []

            def worker(t):
                try:
                    barrier.wait()
                    for _ in range(REP):
                        call(ins[t], outs[t])
                except Exception as e:  # noqa: BLE001
                    errs.append(e)
                    barrier.abort()

            th = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
            [x.start() for x in th]
            [x.join() for x in th]
            ctx.sync()
            assert not errs, errs
            s1 = ctx.CoalescingStats()
        finally:
            if deferred:
                ctx.SetDeferred(0)
            ctx.SetCoalescing(0, 0)
        for t in range(T):
            for k in range(2):
                assert np.array_equal(outs[t][k].get(), want[t][k]), (name, t, k)
        assert s1["calls"] - s0["calls"] == T * REP, (name, s0, s1)


def test_graph_replays_both_directions(ctx):
    S = _queue_setup(ctx, 8700)
    small = [S.ci(uniform_poly(S.rng, S.q, S.n)) for _ in range(2)]
    up, back = [S.std(), S.std()], [S.ci(), S.ci()]
    S.sw.RealToComplex(small, up)  # (plans and the arena are built on first use)
    S.sw.ComplexToReal(up, back)
    want = [o.get() for o in up + back]
    for o in up + back:
        o.Zero()
    with ctx.capture() as g:
        S.sw.RealToComplex(small, up)
        S.sw.ComplexToReal(up, back)
    g.launch()
    ctx.sync()
    assert all(np.array_equal(o.get(), w) for o, w in zip(up + back, want))


def test_trace_replay_of_the_four_entries(ctx):
    S = _queue_setup(ctx, 8800)
    small = [S.ci(uniform_poly(S.rng, S.q, S.n)) for _ in range(2)]
    up, back, un, fo = [S.std(), S.std()], [S.ci(), S.ci()], S.std(), S.ci()

    def run():
        S.sw.RealToComplex(small, up)
        S.sw.ComplexToReal(up, back)
        S.gQ.UnfoldConjugateInvariantToStandard(back[0], un)
        S.gci.FoldStandardToConjugateInvariant(un, fo)

    outs = up + back + [un, fo]
    run()
    ctx.sync()
    want = [o.get() for o in outs]
    for o in outs:
        o.Zero()
    _lib.trace_begin()
    try:
        run()
    finally:
        prog = _lib.trace_end()
    ctx.sync()
    assert all(np.array_equal(o.get(), w) for o, w in zip(outs, want))
    for o in outs:
        o.Zero()
    ctx.sync()
    _lib.replay(ctx.h, prog, 1, 1, [], [], [])
    ctx.sync()
    for i, (o, w) in enumerate(zip(outs, want)):
        assert np.array_equal(o.get(), w), i


# ---- rejections ------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_every_operand_unchanged(ctx):
    S = _queue_setup(ctx, 8900, 14)  # (= 1 mod 2^14: a conjugate-invariant ring of degree N and a standard one of 2N exist)
    q, N, n, nq = S.q, S.N, S.n, S.nq
    level = nq - 1
    rng = S.rng
    g4 = la.Ring(ctx, N // 4, q, conjugate_invariant=True)
    gci_P = la.Ring(ctx, N, S.gP.moduli, conjugate_invariant=True)
    gci_N = la.Ring(ctx, N, q, conjugate_invariant=True)
    ev_ci = la.Evaluator(gci_N, gci_P)                       # an evaluator on a conjugate-invariant ring
    g2N, g2N_P = la.Ring(ctx, 2 * N, q), la.Ring(ctx, 2 * N, S.gP.moduli)
    ev_2N = la.Evaluator(g2N, g2N_P)                         # an evaluator of another degree (and another evaluator for the key)
    ctx2 = la.Context(0)
    other_ctx = la.Poly(la.Ring(ctx2, n, q, conjugate_invariant=True), nq).upload(uniform_poly(rng, q, n))
    big = [S.std(uniform_poly(rng, q, N)) for _ in range(4)]
    small = [S.ci(uniform_poly(rng, q, n)) for _ in range(4)]
    quarter = [la.Poly(g4, nq).upload(uniform_poly(rng, q, N // 4)) for _ in range(2)]
    small_b2 = [S.ci(_rand(rng, q, n, 2), 2) for _ in range(2)]
    short = [S.ci(uniform_poly(rng, q[:2], n), 1, 2) for _ in range(2)]
    allp = big + small + quarter + small_b2 + short + [other_ctx]
    before = [x.download() for x in allp]
    L = _lib.load()
    c2r = lambda ev, lv, i0, i1, k, o0, o1: L.he_complex_to_real(ev.h, lv, i0.h, i1.h, k.h, o0.h, o1.h)
    r2c = lambda ev, lv, i0, i1, k, o0, o1: L.he_real_to_complex(ev.h, lv, i0.h, i1.h, k.h, o0.h, o1.h)
    gev, gk = S.gev, S.gk
    cases = [
        (EINVAL, "ctIn ring degree must be twice", lambda: c2r(gev, level, big[0], big[1], gk, big[2], big[3])),        # ratio 1
        (EINVAL, "ctIn ring degree must be twice", lambda: c2r(gev, level, big[0], big[1], gk, quarter[0], quarter[1])),  # ratio 4
        (EINVAL, "opOut ring degree must be twice", lambda: r2c(gev, level, small[0], small[1], gk, small[2], small[3])),  # ratio 1
        (EINVAL, "opOut ring degree must be twice", lambda: r2c(gev, level, quarter[0], quarter[1], gk, big[2], big[3])),  # ratio 4
        (EINVAL, "not instantiated with RingType ring.Standard", lambda: c2r(ev_ci, level, big[0], big[1], gk, small[2], small[3])),
        (EINVAL, "not instantiated with RingType ring.Standard", lambda: r2c(ev_ci, level, small[0], small[1], gk, big[2], big[3])),
        (EINVAL, "another evaluator", lambda: c2r(ev_2N, level, big[0], big[1], gk, small[2], small[3])),                # a key of another evaluator
        (EINVAL, "does not match evaluator params ring degree", lambda: c2r(gev, level, small[0], small[1], gk, quarter[0], quarter[1])),
        (EINVAL, "does not match evaluator params ring degree", lambda: r2c(gev, level, quarter[0], quarter[1], gk, small[2], small[3])),
        (EINVAL, "batch mismatch", lambda: r2c(gev, level, small_b2[0], small_b2[1], gk, big[2], big[3])),
        (EINVAL, "batch mismatch", lambda: c2r(gev, level, big[0], big[1], gk, small_b2[0], small_b2[1])),
        (EINVAL, "negative level", lambda: c2r(gev, -1, big[0], big[1], gk, small[2], small[3])),                         # level out of range
        (EINVAL, "limbs", lambda: r2c(gev, level, short[0], short[1], gk, big[2], big[3])),                              # level above the operand's limbs
        (EINVAL, "another context", lambda: r2c(gev, level, other_ctx, small[1], gk, big[2], big[3])),
        (EINVAL, "same polynomial", lambda: c2r(gev, level, big[0], big[1], gk, small[2], small[2])),                     # out0 == out1
        (EINVAL, "same polynomial", lambda: r2c(gev, level, small[0], small[1], gk, big[2], big[2])),
        (EINVAL, "differ in degree", lambda: c2r(gev, level, big[0], big[1], gk, small[2], quarter[0])),
        (EHANDLE, "", lambda: c2r(gev, level, big[0], big[1], gk, small[2], S.gQ)),                                      # not a polynomial
        # the ring-level maps
        (EINVAL, "", lambda: L.he_unfold_conjugate_invariant_to_standard(level, small[0].h, small[1].h)),                 # ratio 1
        (EINVAL, "", lambda: L.he_unfold_conjugate_invariant_to_standard(level, quarter[0].h, big[0].h)),                 # ratio 4
        (EINVAL, "", lambda: L.he_unfold_conjugate_invariant_to_standard(level, big[0].h, small[0].h)),                   # the wrong way round
        (EINVAL, "", lambda: L.he_unfold_conjugate_invariant_to_standard(nq, small[0].h, big[0].h)),                      # level
        (EINVAL, "", lambda: L.he_unfold_conjugate_invariant_to_standard(-1, small[0].h, big[0].h)),
        (EINVAL, "", lambda: L.he_fold_standard_to_conjugate_invariant(S.gQ.h, level, big[0].h, quarter[0].h)),           # ratio 4
        (EINVAL, "", lambda: L.he_fold_standard_to_conjugate_invariant(S.gQ.h, level, small[0].h, big[0].h)),             # the wrong way round
        (EINVAL, "", lambda: L.he_fold_standard_to_conjugate_invariant(g4.h, level, big[0].h, small[0].h)),               # ring of another degree
        (EINVAL, "", lambda: L.he_fold_standard_to_conjugate_invariant(S.gQ.h, nq, big[0].h, small[0].h)),                # level
        (EINVAL, "", lambda: L.he_fold_standard_to_conjugate_invariant(S.gQ.h, level, big[0].h, small_b2[0].h)),          # batch
        (EHANDLE, "", lambda: L.he_fold_standard_to_conjugate_invariant(0, level, big[0].h, small[0].h)),                 # no ring
    ]
    for i, (code, text, c) in enumerate(cases):
        assert c() == code, (i, L.he_last_error().decode())
        assert text in L.he_last_error().decode(), (i, L.he_last_error().decode())
    # n = 8 cannot be formed: rings start at logN = 4 (he_ring_create), so no such polynomial reaches the entries
    with pytest.raises(la.HeringError):
        la.Ring(ctx, 8, q, conjugate_invariant=True)
    # accepted: in0 == in1
    assert c2r(gev, level, big[0], big[0], gk, small[2], small[3]) == 0
    ctx.sync()
    ctx2.sync()
    for i, (x, b) in enumerate(zip(allp, before)):
        if x is small[2] or x is small[3]:
            continue  # (written by the accepted call)
        assert np.array_equal(x.download(), b), i
