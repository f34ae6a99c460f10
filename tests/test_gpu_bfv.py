"""BFV scale-invariant MulRelin on the device (include/hering_bfv.h), word for word against the oracle's restatement of the
reference (oracle/circuits.py::ScaleInvariantEvaluator: tensorScaleInvariant / modUpAndNTT / tensorLowDeg / quantize,
schemes/bgv/evaluator.go:898-1071), with the driver sequence of tests/drivers/bgv.py on the same handles as a second leg."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import lattigo_amd as la
from drivers import bgv as DRV
from lattigo_amd import _lib
from lattigo_amd import bfv as BFV
from oracle import circuits as OC
from oracle import oracle as O
from tests import bfv_ref as F
from tests.gpu_common import ctx  # noqa: F401
from tests.helpers import rng_for, uniform_poly
from tests.rlwe_fixtures import downstream_primes
from tests.test_bfv_host import SHAPES, WIDE, chain, word_sets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 65537
EINVAL, EHANDLE = -1, -2


def _rand(rng, q, N, batch):
    return np.stack([uniform_poly(rng, q, N) for _ in range(batch)])


# ---- he_bfv_quantize ---------------------------------------------------------------------------------------------------------------
class QRig:
    """Q and QMul of a host-test shape on both sides, a P-less evaluator (quantize needs no key)"""

    def __init__(self, ctx, logN, shape):
        self.N = 1 << logN
        self.q, self.qm = chain(logN, shape)
        self.gQ, self.gM = la.Ring(ctx, self.N, self.q), la.Ring(ctx, self.N, self.qm)
        self.oQ, self.oM = O.Ring(self.N, self.q), O.Ring(self.N, self.qm)
        self.gs = BFV.ScaleInvariantEvaluator(la.Evaluator(self.gQ, None), self.gM, T)
        self.os = OC.ScaleInvariantEvaluator(O.Evaluator(self.oQ, None), self.oM, T)
        assert self.gs.levelQMul == self.os.levelQMul == F.level_qmul(self.q, logN)

    def check(self, level, sets, names, inplace=False, scratch_out=False):
        """the coefficient-domain word sets of the host test, transformed, through the entry against the oracle's _quantize"""
        lm = self.gs.levelQMul[level]
        oQl, oMl = O.Ring(self.N, self.q[: level + 1]), O.Ring(self.N, self.qm[: lm + 1])
        for name in names:
            cQ, cM = oQl.NTT(sets[name][0]), oMl.NTT(sets[name][1])
            pQ, pM = la.Poly(self.gQ, level + 1).upload(cQ), la.Poly(self.gM, lm + 1).upload(cM)
            out = pQ if inplace else la.Poly(self.gQ, level + 1, 1, zero=not scratch_out)
            self.gs.Quantize(level, pQ, pM, out)
            want = self.os._quantize(level, lm, cQ, cM)
            assert np.array_equal(out.get(), want), (name, level, np.argwhere(out.get() != want)[:4])
            assert np.array_equal(pM.get(), cM) and (inplace or np.array_equal(pQ.get(), cQ)), "inputs unchanged"


@pytest.mark.parametrize("shape", list(SHAPES))
def test_quantize_word_sets(ctx, shape):
    """logN 10: random, all zero, all q - 1 on both sides, and the words that put each float sum within an ulp of an integer; the
    top level, level 0 and the level below the top; once in place"""
    rg = QRig(ctx, 10, shape)
    rng = rng_for(9300 + list(SHAPES).index(shape))
    top = len(rg.q) - 1
    for level in sorted({top, 0, max(top - 1, 0)}):
        lm = rg.gs.levelQMul[level]
        sets = word_sets(rng, F.Quantize(rg.q[: level + 1], rg.qm[: lm + 1], T), rg.N)
        rg.check(level, sets, list(sets))
    rg.check(top, sets, ["random", "ulp"], inplace=True)  # (the sets of the last level of the loop: the top)
    ctx.sync()


@pytest.mark.parametrize("shape", list(WIDE))
def test_quantize_wide_shapes(ctx, shape):
    """one shape per instantiation of the kernel above four limbs of Q, the last at the cap of 32 moduli on both sides; the top
    level and the one below it"""
    rg = QRig(ctx, 10, shape)
    rng = rng_for(9310 + list(WIDE).index(shape))
    top = len(rg.q) - 1
    for level in (top, top - 1):
        lm = rg.gs.levelQMul[level]
        sets = word_sets(rng, F.Quantize(rg.q[: level + 1], rg.qm[: lm + 1], T), rg.N)
        rg.check(level, sets, ["random", "top", "ulp"])
    ctx.sync()


def test_quantize_logn13(ctx):
    rg = QRig(ctx, 13, "4x60|5")
    sets = word_sets(rng_for(9320), F.Quantize(rg.q, rg.qm, T), rg.N)
    rg.check(len(rg.q) - 1, sets, ["random", "ulp"])
    ctx.sync()


def poison_case():
    """run by test_quantize_writes_every_output_word in a process of its own with HERING_POISON=1: the outputs are scratch polynomials"""
    c = la.Context(0)
    for logN, shape in ((10, "3x36|2"), (13, "3|3x61")):
        rg = QRig(c, logN, shape)
        sets = word_sets(rng_for(9330 + logN), F.Quantize(rg.q, rg.qm, T), rg.N)
        rg.check(len(rg.q) - 1, sets, ["random", "top"], scratch_out=True)
    c.sync()


def test_quantize_writes_every_output_word(ctx):
    env = dict(os.environ, HERING_POISON="1")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c",
                        "import tests.conftest; from tests.test_gpu_bfv import poison_case; poison_case()"],  # (conftest: the drivers' path)
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- he_bfv_mul_relin --------------------------------------------------------------------------------------------------------------
def _random_key(rng, q, p, N, pw2=0):
    if pw2:
        nj = [(int(x).bit_length() + pw2 - 1) // pw2 for x in q]
        D = sum(nj)
    else:
        nj, D = None, O.BaseRNSDecompositionVectorSize(len(q) - 1, len(p) - 1)
    kq = np.stack([np.stack([uniform_poly(rng, q, N) for _ in range(2)]) for _ in range(D)])
    kp = np.stack([np.stack([uniform_poly(rng, p, N) for _ in range(2)]) for _ in range(D)])
    return kq, kp, nj


class Rig:
    """the parameters (Q | P) and QMul on both sides, one random relinearisation key (arithmetic parity), the native evaluator, the
    driver and the oracle"""

    def __init__(self, ctx, logN, logq, logp, seed, pw2=0):
        self.ctx, self.N = ctx, 1 << logN
        q, p = O.GenModuli(logN + 1, logq, logp)
        self.q, self.p = [int(x) for x in q], [int(x) for x in p]
        self.rng = rng_for(seed)
        nm = F.level_qmul(self.q, logN)[-1] + 1
        self.qm = downstream_primes(61, 2 * self.N, nm, set(self.q) | set(self.p))
        self.gQ, self.gP, self.gM = la.Ring(ctx, self.N, self.q), la.Ring(ctx, self.N, self.p), la.Ring(ctx, self.N, self.qm)
        self.oQ, self.oP, self.oM = O.Ring(self.N, self.q), O.Ring(self.N, self.p), O.Ring(self.N, self.qm)
        self.gev, self.oev = la.Evaluator(self.gQ, self.gP), O.Evaluator(self.oQ, self.oP)
        kq, kp, nj = _random_key(self.rng, self.q, self.p, self.N, pw2)
        self.gk = self.gev.NewEvaluationKey(kq, kp, pw2, nj) if pw2 else self.gev.NewEvaluationKey(kq, kp)
        self.ok = O.EvaluationKey(kq, kp, pw2=pw2, nj=nj) if pw2 else O.EvaluationKey(kq, kp)
        self.gs = BFV.ScaleInvariantEvaluator(self.gev, self.gM, T)
        self.drv = DRV.ScaleInvariantEvaluator(self.gev, self.gM, T)
        self.os = OC.ScaleInvariantEvaluator(self.oev, self.oM, T)
        self.top = len(self.q) - 1
        assert self.gs.levelQMul == self.os.levelQMul == self.drv.levelQMul

    def ct(self, level, B=1):
        """[B][2][level + 1][N] NTT-domain words"""
        return np.stack([np.stack([uniform_poly(self.rng, self.q[: level + 1], self.N) for _ in range(2)]) for _ in range(B)])

    def up(self, ct):
        B, _, nl, _ = ct.shape
        return [la.Poly(self.gQ, nl, B).upload(ct[:, k]) for k in range(2)]

    def new(self, level, B=1, n=2):
        return [la.Poly(self.gQ, level + 1, B) for _ in range(n)]

    @staticmethod
    def down(polys):
        return np.stack([p.download() for p in polys], axis=1)  # [B][n][limbs][N]

    def want(self, ct0, ct1, key, square=False):
        return np.stack([self.os.MulRelinScaleInvariant(ct0[b], None if square else ct1[b], self.ok if key else None, square=square)
                         for b in range(ct0.shape[0])])


def _mul_case(rg: Rig, level, B, driver_leg=True):
    """with a key, without one (three outputs), the squaring call, in place with out = a and with out = b"""
    ct0, ct1 = rg.ct(level, B), rg.ct(level, B)
    g0, g1 = rg.up(ct0), rg.up(ct1)
    want2, want3, wantsq = rg.want(ct0, ct1, True), rg.want(ct0, ct1, False), rg.want(ct0, None, True, square=True)
    out = rg.new(level, B)
    rg.gs.MulRelinScaleInvariant(level, g0, g1, rg.gk, out)
    assert np.array_equal(Rig.down(out), want2), ("key", level, B)
    out3 = rg.new(level, B, 3)
    rg.gs.MulRelinScaleInvariant(level, g0, g1, None, out3)
    assert np.array_equal(Rig.down(out3), want3), ("no key", level, B)
    outs = rg.new(level, B)
    rg.gs.MulRelinScaleInvariant(level, g0, g0, rg.gk, outs)
    assert np.array_equal(Rig.down(outs), wantsq), ("square", level, B)
    outs3 = rg.new(level, B, 3)
    rg.gs.MulRelinScaleInvariant(level, g0, g0, None, outs3)
    assert np.array_equal(Rig.down(outs3), rg.want(ct0, None, False, square=True)), ("square, no key", level, B)
    assert np.array_equal(Rig.down(g0), ct0) and np.array_equal(Rig.down(g1), ct1), "inputs unchanged"
    if driver_leg:  # the driver sequence on the same handles
        dout, dout3 = rg.new(level, B), rg.new(level, B, 3)
        rg.drv.MulRelinScaleInvariant(level, g0, g1, rg.gk, dout)
        rg.drv.MulRelinScaleInvariant(level, g0, g1, None, dout3)
        assert np.array_equal(Rig.down(dout), Rig.down(out)) and np.array_equal(Rig.down(dout3), Rig.down(out3)), ("driver", level, B)
    # in place: the outputs are the first operand's polynomials, then the second's (crossed: out0 = b1, out1 = b0), then both
    a, b = rg.up(ct0), rg.up(ct1)
    rg.gs.MulRelinScaleInvariant(level, a, b, rg.gk, a)
    assert np.array_equal(Rig.down(a), want2), ("out = a", level, B)
    a = rg.up(ct0)
    rg.gs.MulRelinScaleInvariant(level, a, b, rg.gk, [b[1], b[0]])
    assert np.array_equal(Rig.down([b[1], b[0]]), want2), ("out = b, crossed", level, B)
    a, b = rg.up(ct0), rg.up(ct1)
    rg.gs.MulRelinScaleInvariant(level, a, b, None, [a[0], b[1], a[1]])
    assert np.array_equal(Rig.down([a[0], b[1], a[1]]), want3), ("three outputs over the inputs", level, B)
    a = rg.up(ct0)
    rg.gs.MulRelinScaleInvariant(level, a, a, rg.gk, a)
    assert np.array_equal(Rig.down(a), wantsq), ("square in place", level, B)
    rg.ctx.sync()


SHAPES_MUL = {10: ([55, 45, 45], [55, 55]), 12: ([60, 50, 40, 40], [61]), 13: ([36, 36, 36], [61])}


@pytest.mark.parametrize("logN", list(SHAPES_MUL))
def test_mul_relin_against_the_oracle(ctx, logN):
    """logN 13: three 36-bit moduli of Q, lm + 1 = 2 limbs of QMul -- fewer than Q has"""
    rg = Rig(ctx, logN, *SHAPES_MUL[logN], 9400 + logN)
    if logN == 13:
        assert rg.gs.levelQMul[rg.top] + 1 < len(rg.q)
    _mul_case(rg, rg.top, 1)
    _mul_case(rg, rg.top - 1, 1, driver_leg=False)
    _mul_case(rg, rg.top, 2, driver_leg=logN == 10)


def test_mul_relin_base2_key(ctx):
    rg = Rig(ctx, 12, *SHAPES_MUL[12], 9450, pw2=13)
    _mul_case(rg, rg.top, 1, driver_leg=False)


# ---- launch census -----------------------------------------------------------------------------------------------------------------
def _prof(ctx, call):
    call()  # (plans and the arena are built on first use)
    ctx.sync()
    ctx.prof_begin()
    call()
    ctx.sync()
    return {k: v[0] for k, v in ctx.prof_end().items()}


@pytest.mark.parametrize("B", [1, 2])
def test_launch_census(ctx, B):
    """logN 12, with a key, not squaring: the relinearisation's launches (he_relinearize profiled alone on the same shape) plus the
    transforms (each profiled here as the ring-level call of the same entries), one extension, at most two tensors, one quantize"""
    rg = Rig(ctx, 12, *SHAPES_MUL[12], 9500 + B)
    level, lm = rg.top, rg.gs.levelQMul[rg.top]
    ct0, ct1 = rg.ct(level, B), rg.ct(level, B)
    g0, g1, out = rg.up(ct0), rg.up(ct1), rg.new(level, B)
    L = _lib.load()
    c2 = la.Poly(rg.gQ, level + 1, B).upload(_rand(rg.rng, rg.q, rg.N, B))
    relin = _prof(ctx, lambda: _lib.check(L.he_relinearize(rg.gev.h, level, g0[0].h, g0[1].h, c2.h, rg.gk.h, out[0].h, out[1].h)))
    mul = _prof(ctx, lambda: rg.gs.MulRelinScaleInvariant(level, g0, g1, rg.gk, out))
    sq = _prof(ctx, lambda: rg.gs.MulRelinScaleInvariant(level, g0, g0, rg.gk, out))
    rQ, rM = rg.gQ.AtLevel(level), rg.gM.AtLevel(lm)
    pQ1, pQ3 = la.Poly(rg.gQ, level + 1, B), la.Poly(rg.gQ, level + 1, 3 * B)
    pM4, pM3 = la.Poly(rg.gM, lm + 1, 4 * B), la.Poly(rg.gM, lm + 1, 3 * B)
    n = lambda d: sum(d.values())
    budget = (4 * n(_prof(ctx, lambda: rQ.INTT(pQ1, pQ1))) + n(_prof(ctx, lambda: rM.NTTLazy(pM4, pM4)))
              + n(_prof(ctx, lambda: rQ.INTT(pQ3, pQ3))) + n(_prof(ctx, lambda: rM.INTT(pM3, pM3)))
              + n(_prof(ctx, lambda: rQ.NTT(pQ3, pQ3))) + 4)
    print("relinearize", relin, "\nmul_relin", mul, "\nsquare", sq, "\nbudget beyond the relinearisation", budget)
    assert mul.get("bfv_quantize") == 1 and "bfv_quantize" not in relin
    assert 1 <= mul.get("tensor", 0) <= 2
    assert mul.get("modup", 0) == relin.get("modup", 0) + 1
    assert mul.get("ew", 0) == relin.get("ew", 0)
    assert n(mul) - n(relin) <= budget, (n(mul), n(relin), budget)
    assert n(sq) < n(mul)
    # the driver's train on the same handles, for the record
    drv = _prof(ctx, lambda: rg.drv.MulRelinScaleInvariant(level, g0, g1, rg.gk, out))
    print("driver", n(drv), "launches against", n(mul))
    assert n(mul) < n(drv)


# ---- the submission queue, graphs and replay -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("deferred", [0, 4])
def test_queue_coalesced_and_deferred(ctx, deferred):
    """8 threads on their own batch-1 handles; bit-identical to the direct calls (the requests are served one by one)"""
    rg = Rig(ctx, 10, *SHAPES_MUL[10], 9600 + deferred)
    level, TH, REP = rg.top, 8, 2
    data = [(rg.ct(level), rg.ct(level)) for _ in range(TH)]
    want = []
    for a, b in data:
        out = rg.new(level)
        rg.gs.MulRelinScaleInvariant(level, rg.up(a), rg.up(b), rg.gk, out)
        want.append(Rig.down(out))
    ctx.sync()
    ins = [(rg.up(a), rg.up(b)) for a, b in data]
    outs = [rg.new(level) for _ in range(TH)]
    ctx.SetCoalescing(64, 2000)
    if deferred:
        ctx.SetDeferred(deferred)
    try:
        s0 = ctx.CoalescingStats()
        barrier, errs = threading.Barrier(TH), []

        def worker(t):
            try:
                barrier.wait()
                for _ in range(REP):
                    rg.gs.MulRelinScaleInvariant(level, ins[t][0], ins[t][1], rg.gk, outs[t])
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
        assert np.array_equal(Rig.down(outs[t]), want[t]), t
    assert s1["calls"] - s0["calls"] == TH * REP, (s0, s1)


def _three_calls(rg, level, g0, g1, out, out3, qout, pM):
    rg.gs.MulRelinScaleInvariant(level, g0, g1, rg.gk, out)
    rg.gs.MulRelinScaleInvariant(level, g0, g1, None, out3)
    rg.gs.Quantize(level, out3[2], pM, qout)


def _replay_setup(ctx, seed):
    rg = Rig(ctx, 10, *SHAPES_MUL[10], seed)
    level = rg.top
    lm = rg.gs.levelQMul[level]
    g0, g1 = rg.up(rg.ct(level)), rg.up(rg.ct(level))
    out, out3, qout = rg.new(level), rg.new(level, 1, 3), la.Poly(rg.gQ, level + 1)
    pM = la.Poly(rg.gM, lm + 1).upload(uniform_poly(rg.rng, rg.qm[: lm + 1], rg.N))
    run = lambda: _three_calls(rg, level, g0, g1, out, out3, qout, pM)
    return rg, run, out + out3 + [qout]


def test_graph_capture_and_launch(ctx):
    rg, run, outs = _replay_setup(ctx, 9700)
    run()  # (plans and the arena are built on first use)
    ctx.sync()
    want = [o.get() for o in outs]
    for o in outs:
        o.Zero()
    with ctx.capture() as g:
        run()
    g.launch()
    ctx.sync()
    assert all(np.array_equal(o.get(), w) for o, w in zip(outs, want))


def test_trace_replay_round_trip(ctx):
    rg, run, outs = _replay_setup(ctx, 9800)
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


# ---- rejections ----------------------------------------------------------------------------------------------------------------------
def test_rejections_leave_every_operand_unchanged(ctx):
    rg = Rig(ctx, 10, *SHAPES_MUL[10], 9900)
    level, N = rg.top, rg.N
    L = _lib.load()
    ins = rg.up(rg.ct(level)) + rg.up(rg.ct(level))
    outs = [la.Poly(rg.gQ, level + 1).upload(uniform_poly(rg.rng, rg.q, N)) for _ in range(3)]
    short = la.Poly(rg.gQ, level).upload(uniform_poly(rg.rng, rg.q[:level], N))
    b2 = la.Poly(rg.gQ, level + 1, 2).upload(_rand(rg.rng, rg.q, N, 2))
    allp = ins + outs + [short, b2]
    before = [x.download() for x in allp]
    mul = lambda lv, a0, a1, b0, b1, k, o0, o1, o2: L.he_bfv_mul_relin(rg.gs.h, lv, a0.h, a1.h, b0.h, b1.h, k, o0.h, o1.h, o2)
    k = rg.gk.h
    # a key that stops below the level
    kq, kp, _ = _random_key(rg.rng, rg.q[:level], rg.p, N)
    low = rg.gev.NewEvaluationKey(kq, kp)
    cases = [
        (EINVAL, "same polynomial", lambda: mul(level, *ins, k, outs[0], outs[0], 0)),                    # out0 == out1
        (EINVAL, "same polynomial", lambda: mul(level, *ins, 0, outs[0], outs[1], outs[1].h)),            # out1 == out2
        (EINVAL, "out of range", lambda: mul(level + 1, *ins, k, outs[0], outs[1], 0)),                   # a level above the top
        (EINVAL, "out of range", lambda: mul(-1, *ins, k, outs[0], outs[1], 0)),
        (EINVAL, "limbs", lambda: mul(level, short, ins[1], ins[2], ins[3], k, outs[0], outs[1], 0)),     # too few limbs, an input
        (EINVAL, "limbs", lambda: mul(level, *ins, k, outs[0], short, 0)),                                # ... an output
        (EINVAL, "batch mismatch", lambda: mul(level, *ins, k, outs[0], b2, 0)),
        (EHANDLE, "", lambda: mul(level, *ins, 0, outs[0], outs[1], 0)),                                  # no key: out2 is required
        (EINVAL, "below ciphertext level", lambda: mul(level, *ins, low.h, outs[0], outs[1], 0)),
        (EHANDLE, "", lambda: L.he_bfv_mul_relin(rg.gev.h, level, *[x.h for x in ins], k, outs[0].h, outs[1].h, 0)),  # not a BFV evaluator
        (EINVAL, "same polynomial", lambda: L.he_bfv_quantize(rg.gs.h, level, outs[0].h, outs[1].h, outs[1].h)),      # outQ == cM
        (EINVAL, "out of range", lambda: L.he_bfv_quantize(rg.gs.h, level + 1, outs[0].h, outs[1].h, outs[2].h)),
    ]
    for i, (code, text, c) in enumerate(cases):
        assert c() == code, (i, L.he_last_error().decode())
        assert text in L.he_last_error().decode(), (i, L.he_last_error().decode())
    # the evaluator: a ringQMul that is too short, of another degree, of the other ring type, sharing a modulus, of another context
    h = _lib.H()
    import ctypes as C
    create = lambda ev, ring, t=T: L.he_bfv_evaluator_create(ev.h, ring.h, t, C.byref(h))
    q2 = [int(x) for x in O.GenModuli(12, [61, 61], [])[0]]
    ctx2 = la.Context(0)
    ci_ev = la.Evaluator(la.Ring(ctx, N, q2, conjugate_invariant=True), None)
    for code, text, c in [
        (EINVAL, "levelQMul at the top level", lambda: create(rg.gev, la.Ring(ctx, N, rg.qm[:-1]))),
        (EINVAL, "degree", lambda: create(rg.gev, la.Ring(ctx, 2 * N, [int(x) for x in O.GenModuli(12, [61] * len(rg.qm), [])[0]]))),
        (EINVAL, "conjugate-invariant", lambda: create(rg.gev, la.Ring(ctx, N, q2, conjugate_invariant=True))),
        (EINVAL, "conjugate-invariant", lambda: create(ci_ev, rg.gM)),
        (EINVAL, "another context", lambda: create(rg.gev, la.Ring(ctx2, N, rg.qm))),
        (EINVAL, "zero", lambda: create(rg.gev, rg.gM, 0)),
        (-4, "share a modulus", lambda: create(rg.gev, la.Ring(ctx, N, rg.qm[:-1] + rg.q[:1]))),
        (EHANDLE, "", lambda: create(rg.gQ, rg.gM)),
    ]:
        assert c() == code, (text, L.he_last_error().decode())
        assert text in L.he_last_error().decode(), (text, L.he_last_error().decode())
    lm = C.c_int()
    assert L.he_bfv_level_qmul(rg.gs.h, level + 1, C.byref(lm)) == EINVAL
    ctx.sync()
    ctx2.sync()
    for i, (x, b) in enumerate(zip(allp, before)):
        assert np.array_equal(x.download(), b), i
