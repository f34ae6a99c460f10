"""Blind rotation on the device (include/hering_blindrot.h, lattigo_amd.blindrot): he_automorphism_ct_select word for word against
the oracle's Automorphism, he_blind_rotate_core and Evaluate against tests/blindrot_ref.py -- core/rgsw/blindrot/evaluator.go
restated on the oracle -- at the smallest shapes at which each route can still go wrong."""
import ctypes as C
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd import _lib
from lattigo_amd import blindrot as B
from lattigo_amd import rgsw as G
from oracle import oracle as O
from tests import blindrot_ref as BR
from tests import rgsw_edges as E
from tests import rgsw_ref as R
from tests import rlwe_fixtures as F
from tests.gpu_common import ctx  # noqa: F401
from tests.helpers import rng_for, uniform_poly

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
K_AUTO, K_PROD = "automorphism_ct_select", "rgsw_external_product"
Q27 = 0x7FFF801  # the reference's blind rotation modulus (blindrot_test.go:55)


@pytest.fixture(autouse=True)
def _no_garbage_left_behind():
    gc.collect()
    yield
    gc.collect()


class Setup:
    """One parameter set on both sides, with uniformly random RGSW and Galois keys."""

    def __init__(self, ctx, logN, q, p, pw2, ci=False):
        self.logN, self.N, self.q, self.p, self.pw2 = logN, 1 << logN, list(q), list(p), pw2
        self.oQ = O.Ring(self.N, self.q, ci)
        self.oP = O.Ring(self.N, self.p, ci) if self.p else None
        self.oev = O.Evaluator(self.oQ, self.oP)
        self.gQ = la.Ring(ctx, self.N, self.q, conjugate_invariant=ci)
        self.gP = la.Ring(ctx, self.N, self.p, conjugate_invariant=ci) if self.p else None
        self.gev = G.Evaluator(self.gQ, self.gP)
        self.level = len(self.q) - 1

    def key(self, o):
        kw = dict(BaseTwoDecomposition=o.pw2, BaseTwoDecompositionVectorSize=o.nj) if o.pw2 else {}
        return self.gev.NewEvaluationKey(o.q, o.p if self.p else None, **kw)

    def galois(self, rng, gal_els, pw2=None):
        """({Galois element: oracle key}, device GaloisKeySet) with uniformly random words"""
        pw2 = self.pw2 if pw2 is None else pw2
        okeys = {}
        for g in gal_els:
            okeys[int(g)] = R.uniform_rgsw(rng, self.oQ, self.oP, pw2)[0]
        return okeys, B.GaloisKeySet(self.gev, {g: self.key(o) for g, o in okeys.items()})

    def rgsw(self, rng, n):
        """([oracle RGSW pairs], [device rgsw.Ciphertext])"""
        o = [R.uniform_rgsw(rng, self.oQ, self.oP, self.pw2) for _ in range(n)]
        return o, [G.Ciphertext(self.key(k[0]), self.key(k[1])) for k in o]

    def cts(self, rng, batch):
        return np.stack([np.stack([uniform_poly(rng, self.q, self.N) for _ in range(2)]) for _ in range(batch)])

    def up(self, ct):
        return [la.Poly(self.gQ, ct.shape[2], ct.shape[0]).upload(np.ascontiguousarray(ct[:, k])) for k in range(2)]

    def down(self, polys):
        return np.stack([p.download()[:, : self.level + 1] for p in polys], axis=1)

    def new_ct(self, batch):
        return [la.Poly(self.gQ, self.level + 1, batch) for _ in range(2)]


# ---- 1. he_automorphism_ct_select ---------------------------------------------------------------------------------------------
SEL = [0, -1, 10, 3, 3]


def _select_shapes():
    out = {}
    for logN in (9, 10, 11):
        out[f"{logN}-q27-pw2-7"] = (logN, [Q27] if logN == 10 else [O.GenModuli(logN + 1, [27], [])[0][0]], [], 7)
    q, p = E.moduli(9, (35, 20), (61,))
    out["9-35-20-P61-pw2-7"] = (9, q, p, 7)
    out["9-35-20-P61-pw2-13"] = (9, q, p, 13)
    out["9-35-14-P61-pw2-14-window-reaches-q"] = (9, [q[0], E.Q14], p, 14)  # mask 16383 >= 12289
    return out


SELECT_SHAPES = _select_shapes()


def _inputs(kind, S, rng, batch):
    ct = S.cts(rng, batch)
    if kind == "q-1":
        for i, q in enumerate(S.q):
            ct[:, :, i] = np.uint64(q - 1)
    elif kind == "in1-lazy":
        for i, q in enumerate(S.q):
            ct[:, 1, i] += np.uint64(q)
    return ct


def _want_select(S, ct, okeys, gal_els, sel):
    return np.stack([ct[b] if s < 0 else S.oev.Automorphism(ct[b], gal_els[s], okeys[gal_els[s]]) for b, s in enumerate(sel)])


@pytest.mark.parametrize("kind", ["random", "q-1", "in1-lazy"])
@pytest.mark.parametrize("shape", sorted(SELECT_SHAPES))
def test_automorphism_select(ctx, shape, kind):
    logN, q, p, pw2 = SELECT_SHAPES[shape]
    S = Setup(ctx, logN, q, p, pw2)
    rng = rng_for(9600 + len(shape) + len(kind))
    gal_els = BR.galois_elements(S.N)
    assert len(gal_els) == 11 and gal_els[10] == 2 * S.N - 5
    okeys, dset = S.galois(rng, gal_els)
    if pw2 == 14:
        assert (1 << pw2) - 1 >= E.Q14
    ct = _inputs(kind, S, rng, len(SEL))
    want = _want_select(S, ct, okeys, gal_els, SEL)
    op0, out = S.up(ct), S.new_ct(len(SEL))
    B.AutomorphismSelect(S.gev, op0, dset, SEL, out)
    assert np.array_equal(S.down(out), want)
    assert np.array_equal(S.down(op0), ct), "the inputs were changed"
    B.AutomorphismSelect(S.gev, op0, dset, SEL, op0)  # in place
    assert np.array_equal(S.down(op0), want)


def test_automorphism_select_is_one_launch_and_shares_in0_in1(ctx):
    logN, q, p, pw2 = SELECT_SHAPES["9-35-20-P61-pw2-7"]
    S = Setup(ctx, logN, q, p, pw2)
    rng = rng_for(9650)
    gal_els = BR.galois_elements(S.N)
    okeys, dset = S.galois(rng, gal_els)
    ct = S.cts(rng, len(SEL))
    ct[:, 1] = ct[:, 0]
    want = _want_select(S, ct, okeys, gal_els, SEL)
    one = la.Poly(S.gQ, S.level + 1, len(SEL)).upload(np.ascontiguousarray(ct[:, 0]))
    out = S.new_ct(len(SEL))
    B.AutomorphismSelect(S.gev, [one, one], dset, SEL, out)  # in0 == in1
    assert np.array_equal(S.down(out), want)
    ctx.sync()
    ctx.prof_begin()
    B.AutomorphismSelect(S.gev, [one, one], dset, SEL, out)
    prof = ctx.prof_end()
    assert prof[K_AUTO][0] == 1 and sum(n for n, _ in prof.values()) == 1, prof


def test_automorphism_select_rejections(ctx):
    logN, q, p, pw2 = SELECT_SHAPES["9-35-20-P61-pw2-7"]
    S = Setup(ctx, logN, q, p, pw2)
    rng = rng_for(9660)
    gal_els = BR.galois_elements(S.N)
    _, dset = S.galois(rng, gal_els)
    ct = S.cts(rng, 5)
    op0, out = S.up(ct), S.up(ct)
    L = _lib.load()

    def rc(ev, i0, i1, ds, sel, o0, o1):
        s = (C.c_int32 * len(sel))(*sel)
        return L.he_automorphism_ct_select(ev.h, i0.h, i1.h, ds.h, s, len(sel), o0.h, o1.h)

    assert rc(S.gev, op0[0], op0[1], dset, [0, -1, 11, 3, 3], out[0], out[1]) == EINVAL   # sel out of range
    assert rc(S.gev, op0[0], op0[1], dset, [0, -2, 10, 3, 3], out[0], out[1]) == EINVAL
    assert rc(S.gev, op0[0], op0[1], dset, [0, -1, 10, 3], out[0], out[1]) == EINVAL      # n_sel != batch
    assert rc(S.gev, op0[0], op0[1], dset, SEL, out[0], out[0]) == EINVAL                 # out0 == out1
    assert rc(S.gev, op0[0], op0[1], dset, SEL, op0[1], out[1]) == EINVAL                 # out0 == in1
    # a BaseTwoDecomposition = 0 key: the centred decomposition is not in the kernel's domain
    _, dset0 = S.galois(rng, gal_els[:2], pw2=0)
    assert rc(S.gev, op0[0], op0[1], dset0, [0, 1, -1, 0, 0], out[0], out[1]) == EINVAL
    # a shape outside the one-launch domain: logN 8
    q8, p8 = E.moduli(8, (35, 20), (61,))
    S8 = Setup(ctx, 8, q8, p8, 7)
    _, dset8 = S8.galois(rng, BR.galois_elements(S8.N)[:2])
    ct8 = S8.cts(rng, 2)
    op8, out8 = S8.up(ct8), S8.up(ct8)
    assert rc(S8.gev, op8[0], op8[1], dset8, [0, 1], out8[0], out8[1]) == EINVAL
    assert rc(S.gev, op0[0], op0[1], dset8, SEL, out[0], out[1]) == EINVAL                # a set of another evaluator
    assert np.array_equal(S.down(out), ct) and np.array_equal(S.down(op0), ct)
    assert np.array_equal(S8.down(out8), ct8) and np.array_equal(S8.down(op8), ct8)


# ---- 2. he_blind_rotate_core against the restatement -------------------------------------------------------------------------------
N_LWE = 16


def _rows(rng, N, n_lwe):
    """five rows mod 2N: random ones, one with all a[i] equal and one with 0, 1 and 2N - 1"""
    odd = lambda n: (rng.integers(0, N, size=n) * 2 + 1).astype(np.uint64)
    rows = [odd(n_lwe), odd(n_lwe), np.full(n_lwe, int(odd(1)[0]), dtype=np.uint64), odd(n_lwe), odd(n_lwe)]
    rows[3][:3] = [0, 1, 2 * N - 1]
    return np.stack(rows)


class CoreCase:
    """keys, five rows, accumulators and the restatement's results at one shape: computed once per module"""

    def __init__(self, ctx, logN, q, p, pw2, n_lwe, batch, seed):
        self.S = S = Setup(ctx, logN, q, p, pw2)
        rng = rng_for(seed)
        self.gal_els = BR.galois_elements(S.N)
        self.ogks, self.dgks = S.galois(rng, self.gal_els)
        self.obrk, dbrk = S.rgsw(rng, n_lwe)
        self.BRK = B.MemBlindRotationEvaluationKeySet.__new__(B.MemBlindRotationEvaluationKeySet)
        self.BRK.BlindRotationKeys, self.BRK.AutomorphismKeys = dbrk, None
        self.BRK.rgsw, self.BRK.galois = S.gev.NewKeySet(dbrk), self.dgks
        self.rows = _rows(rng, S.N, n_lwe)[:batch]
        self.acc = S.cts(rng, batch)
        self.want = np.stack([BR.blind_rotate_core(S.oev, self.rows[b], self.acc[b], self.obrk, self.ogks) for b in range(batch)])
        self.ev = B.Evaluator(S.gev, S.gQ)


@pytest.fixture(scope="module")
def core512(ctx):
    return CoreCase(ctx, 9, [Q27], [], 7, N_LWE, 5, 9700)


@pytest.mark.parametrize("batch", [1, 5])
def test_core_against_restatement(ctx, core512, batch):
    c = core512
    acc = c.S.up(c.acc[:batch])
    c.ev.BlindRotateCore(c.rows[:batch], acc, c.BRK)
    assert np.array_equal(c.S.down(acc), c.want[:batch])


@pytest.mark.parametrize("n_lwe", [1, 7])
def test_core_rows_shorter_than_the_rgsw_set(ctx, core512, n_lwe):
    """n_lwe = 1, and n_lwe below the sixteen keys of the RGSW set: the first n_lwe words of every row and the first n_lwe keys"""
    c = core512
    rows = np.ascontiguousarray(c.rows[:, :n_lwe])
    assert n_lwe < len(c.obrk) == N_LWE and rows.shape == (5, n_lwe)
    want = np.stack([BR.blind_rotate_core(c.S.oev, rows[b], c.acc[b], c.obrk, c.ogks) for b in range(5)])
    acc = c.S.up(c.acc)
    c.ev.BlindRotateCore(rows, acc, c.BRK)
    assert np.array_equal(c.S.down(acc), want)


@pytest.mark.parametrize("switch", ["HERING_NO_BLINDROT_BATCH", "HERING_NO_RGSW_FUSED"])
def test_core_per_entry_routes(switch):
    env = dict(os.environ)
    env[switch] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        "tests/test_gpu_blindrot.py::test_core_against_restatement", "tests/test_gpu_blindrot.py::test_launch_census"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout + r.stderr)[-1500:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "failed" not in r.stdout, tail


def test_core_rejections(ctx, core512):
    c = core512
    acc = c.S.up(c.acc[:2])
    rows = c.rows[:2].copy()
    rows[1, 5] = 6  # even and not zero: the reference panics
    with pytest.raises(la.HeringError) as e:
        c.ev.BlindRotateCore(rows, acc, c.BRK)
    assert e.value.code == EINVAL
    with pytest.raises(la.HeringError):  # rows for another batch
        c.ev.BlindRotateCore(c.rows[:3], acc, c.BRK)
    with pytest.raises(la.HeringError):  # more words than blind rotation keys
        c.ev.BlindRotateCore(np.ones((2, N_LWE + 1), dtype=np.uint64), acc, c.BRK)
    L = _lib.load()
    r = np.ascontiguousarray(c.rows[:2])
    assert L.he_blind_rotate_core(c.S.gev.h, r.ctypes.data_as(_lib.u64p), 2, N_LWE, acc[0].h, acc[0].h, c.BRK.rgsw.h, c.BRK.galois.h) == EINVAL
    assert np.array_equal(c.S.down(acc), c.acc[:2])


# ---- 3. shapes of the per-entry route only ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logp,pw2", [((61,), 7), ((61, 61), 0)], ids=["logN8-P-pw2-7", "logN8-two-P-rns-gadget"])
def test_core_outside_the_one_launch_domain(ctx, logp, pw2):
    q, p = E.moduli(8, (35, 20), logp)
    c = CoreCase(ctx, 8, q, p, pw2, 4, 2, 9750 + pw2)
    acc = c.S.up(c.acc)
    ctx.sync()
    ctx.prof_begin()
    c.ev.BlindRotateCore(c.rows, acc, c.BRK)
    prof = ctx.prof_end()
    assert K_AUTO not in prof and K_PROD not in prof, prof
    assert np.array_equal(c.S.down(acc), c.want)


# ---- 4. launch census -----------------------------------------------------------------------------------------------------------------
def _kernel_launches(ctx, c, rows, acc):
    c.ev.BlindRotateCore(rows, acc, c.BRK)  # (the scratch arena is sized on first use)
    ctx.sync()
    ctx.prof_begin()
    c.ev.BlindRotateCore(rows, acc, c.BRK)
    prof = ctx.prof_end()
    return prof


def test_launch_census(ctx, core512):
    c = core512
    batched = not (os.environ.get("HERING_NO_BLINDROT_BATCH") or os.environ.get("HERING_NO_RGSW_FUSED"))
    rounds = B.Rounds(c.S.logN, c.rows)
    n_auto = sum(1 for g, _ in rounds if np.any(g != 0))
    n_prod = sum(1 for _, p in rounds if np.any(p >= 0))
    prof = _kernel_launches(ctx, c, c.rows, c.S.up(c.acc))
    if not batched:
        assert K_AUTO not in prof, prof
        return
    # the selection's fills are not profiled kernels: the census is the non-empty launches of the rounds
    assert prof[K_AUTO][0] == n_auto and prof[K_PROD][0] == n_prod and sum(n for n, _ in prof.values()) == n_auto + n_prod, prof
    lens = [BR.rounds_of(BR.schedule(c.S.N, r)) for r in c.rows]
    longest = int(np.argmax(lens))
    assert len(rounds) == max(lens) and n_auto + n_prod <= 2 * max(lens)
    # the longest entry alone, and five copies of it: the same launches, whatever the batch
    row = c.rows[longest:longest + 1]
    one = _kernel_launches(ctx, c, row, c.S.up(c.acc[:1]))
    five = _kernel_launches(ctx, c, np.repeat(row, 5, axis=0), c.S.up(c.acc))
    count = lambda p: (p[K_AUTO][0], p[K_PROD][0], sum(n for n, _ in p.values()))
    ops = BR.schedule(c.S.N, row[0])
    assert count(one) == count(five) == (sum(k == BR.AUTO for k, _ in ops), sum(k == BR.PROD for k, _ in ops), len(ops))


# ---- 5. Evaluate end to end, real keys -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real_keys(ctx):
    rng = rng_for(9800)
    S = Setup(ctx, 9, [Q27], [], 7)
    rL = O.Ring(N_LWE, [0x3001])
    sk, skl = F.SecretKey(rng, S.oQ, None), F.SecretKey(rng, rL, None)
    obrk, ogks = BR.gen_blind_rotation_keys(rng, S.oQ, None, sk, skl.vals, 7)
    slots = 8
    values = [-1 + 2 * i / slots for i in range(slots)]
    ct = BR.encrypt_lwe_values(rng, rL, skl, values, 0x3001 / 4.0)
    return dict(S=S, rL=rL, sk=sk, obrk=obrk, ogks=ogks, values=values, ct=ct)


@pytest.mark.parametrize("ntt_flag", [True, False], ids=["NTTFlag", "coefficients"])
def test_evaluate_end_to_end(ctx, real_keys, ntt_flag):
    k = real_keys
    S, rL = k["S"], k["rL"]
    scaleBR = Q27 / 4.0
    otest = BR.init_test_polynomial(BR.sign, scaleBR, S.oQ, -1, 1)
    want = BR.evaluate(S.oev, rL, k["ct"], {i: otest for i in range(len(k["values"]))}, k["obrk"], k["ogks"], ntt_flag)
    gL = la.Ring(ctx, N_LWE, [0x3001])
    dtest = B.InitTestPolynomial(BR.sign, scaleBR, S.gQ, -1, 1)
    assert np.array_equal(dtest.download()[0], otest)
    BRK = B.MemBlindRotationEvaluationKeySet(S.gev, [G.Ciphertext(S.key(o[0]), S.key(o[1])) for o in k["obrk"]],
                                             {g: S.key(o) for g, o in k["ogks"].items()})
    ev = B.Evaluator(S.gev, gL, NTTFlag=ntt_flag)
    dct = [la.Poly(gL, 1, 1).upload(k["ct"][c][None]) for c in range(2)]
    res = ev.Evaluate(dct, {i: dtest for i in range(len(k["values"]))}, BRK)
    assert sorted(res) == sorted(want)
    for i, v in enumerate(k["values"]):
        got = np.stack([p.download()[0] for p in res[i]])
        assert np.array_equal(got, want[i]), i
        if v != 0:
            a = BR.decode(S.oQ, got, k["sk"], scaleBR, is_ntt=ntt_flag)
            assert round(a * 8) / 8 == BR.sign(v), (i, v, a)


# ---- 6. call modes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["queue", "deferred", "graph", "replay"])
def test_core_call_modes(ctx, core512, mode):
    c = core512
    rows, start, want = c.rows[:2], c.acc[:2], c.want[:2]
    acc = c.S.up(start)
    c.ev.BlindRotateCore(rows, acc, c.BRK)  # (sizes the scratch arena)
    ctx.sync()
    fresh = c.S.up(start)
    reset = lambda: [a.CopyLvl(c.S.level, s) for a, s in zip(acc, fresh)]
    reset()
    ctx.sync()
    if mode in ("queue", "deferred"):
        ctx.SetCoalescing(64, 2000)
        if mode == "deferred":
            ctx.SetDeferred(8)
        try:
            r = rows.copy()
            c.ev.BlindRotateCore(r, acc, c.BRK)
            r[:] = 1  # the rows are read during the call
            ctx.sync()
        finally:
            if mode == "deferred":
                ctx.SetDeferred(0)
            ctx.SetCoalescing(0, 0)
        assert np.array_equal(c.S.down(acc), want)
    elif mode == "graph":
        r = rows.copy()
        with ctx.capture() as g:
            c.ev.BlindRotateCore(r, acc, c.BRK)
        r[:] = 1  # frozen in the graph
        for _ in range(2):
            reset()
            g.launch()
            ctx.sync()
            assert np.array_equal(c.S.down(acc), want)
        g.close()
    else:
        _lib.trace_begin()
        try:
            c.ev.BlindRotateCore(rows, acc, c.BRK)
        finally:
            prog = _lib.trace_end()
        ctx.sync()
        assert np.array_equal(c.S.down(acc), want)
        reset()
        ctx.sync()
        _lib.replay(ctx.h, prog, 1, 1, [], [], [])
        ctx.sync()
        assert np.array_equal(c.S.down(acc), want)
