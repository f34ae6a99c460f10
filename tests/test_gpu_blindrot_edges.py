"""The one-launch automorphism (he_automorphism_ct_select) and the batched blind rotation (he_blind_rotate_core) at the edges of
their domain, words, moduli and schedules (include/hering_blindrot.h), word for word against the oracle's Automorphism and
tests/blindrot_ref.py.  tests/test_gpu_blindrot.py holds both with uniformly random words at a few shapes; this file plants the
values and builds the shapes and rows at which the automorphism's instantiation of gadget_fused_kernel -- the RGSW product's
kernel body with one decomposed component and a tail of its own -- and the batched route's selection table can be wrong
without those tests noticing (tests/blindrot_edges.py builds them, tests/test_blindrot_host.py checks without a device that each
has the property it is built for).  Every case that claims the one-launch route asserts it from the launch profile before any
word is compared: one launch of "automorphism_ct_select" and nothing else."""
import ctypes as C
import gc
import itertools
from types import SimpleNamespace

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd import _lib
from lattigo_amd import blindrot as B
from lattigo_amd import rgsw as G
from tests import blindrot_aliasing as BA
from tests import blindrot_edges as BE
from tests import blindrot_ref as BR
from tests import boundary as Bd
from tests import rgsw_edges as E
from tests import rgsw_ref as R
from tests.gpu_common import ctx  # noqa: F401
from tests.helpers import rng_for, uniform_poly
from tests.test_gpu_blindrot import EINVAL, K_AUTO, K_PROD
from tests.test_gpu_rgsw import Setup as RgswSetup
from tests.test_gpu_rgsw_edges import _run_at_level, _select_batch

pytestmark = pytest.mark.gpu

SEL = [0, -1, 1, 0]  # a pass-through entry between working ones


@pytest.fixture(autouse=True)
def _no_garbage_left_behind():
    gc.collect()
    yield
    gc.collect()


class Routed:
    """rgsw.Evaluator whose select automorphisms assert the one-launch route from the launch profile"""

    def __init__(self, ev, ctx):
        self._ev, self._ctx, self.prof = ev, ctx, None

    def __getattr__(self, name):
        if name.startswith("_"):  # (never forward a lookup of the wrapper's own fields: it would recurse)
            raise AttributeError(name)
        return getattr(self._ev, name)

    def AutomorphismSelect(self, op0, dset, sel, opOut):
        self._ctx.sync()
        self._ctx.prof_begin()
        try:
            B.AutomorphismSelect(self._ev, op0, dset, sel, opOut)
        finally:
            self.prof = self._ctx.prof_end()
        # (the selection's fills are not profiled kernels: the kernel's one launch is the whole profile)
        assert set(self.prof) == {K_AUTO} and self.prof[K_AUTO][0] == 1, self.prof


class Edge(RgswSetup):
    """One parameter set on both sides with Galois keys below the ring's top level, chosen window counts and other word sources"""

    def __init__(self, ctx, logN, q, p, pw2, nj=None, level=None, ci=False, key_words=None, in0_words=None, in1_words=None):
        super().__init__(ctx, logN, q, p, pw2, ci)
        self.ctx, self.logN = ctx, logN
        self.gev = Routed(self.gev, ctx)
        self.nj, self.key_words, self.in0_words, self.in1_words = nj, key_words, in0_words, in1_words
        if level is not None:
            self.level = level

    def okey(self, rng):
        return R.uniform_rgsw(rng, self.oQ, self.oP, self.pw2, levelQ=self.level, nj=self.nj, words=self.key_words)[0]

    def dkey(self, o):
        kw = dict(BaseTwoDecomposition=o.pw2, BaseTwoDecompositionVectorSize=o.nj) if o.pw2 else {}
        return self.gev.NewEvaluationKey(o.q, o.p if self.p else None, **kw)

    def galois_set(self, okeys):
        """{Galois element: oracle key} -> device GaloisKeySet, keys in the dict's order"""
        return B.GaloisKeySet(self.gev._ev, {g: self.dkey(o) for g, o in okeys.items()})

    def galois(self, rng, gal_els=None):
        okeys = {int(g): self.okey(rng) for g in (gal_els or BE.galois_pair(self.N))}
        return okeys, self.galois_set(okeys)

    def rgsw_set(self, rng, n):
        o = [R.uniform_rgsw(rng, self.oQ, self.oP, self.pw2, levelQ=self.level, nj=self.nj) for _ in range(n)]
        d = [G.Ciphertext(self.dkey(k[0]), self.dkey(k[1])) for k in o]
        return o, d, self.gev.NewKeySet(d)

    def cts(self, rng, batch):
        mods = self.q[: self.level + 1]
        s0, s1 = self.in0_words or uniform_poly, self.in1_words or uniform_poly
        return np.stack([np.stack([s0(rng, mods, self.N), s1(rng, mods, self.N)]) for _ in range(batch)])

    def want_select(self, ct, okeys, sel):
        gal = list(okeys)
        return np.stack([ct[b] if s < 0 else self.oev.Automorphism(ct[b], gal[s], okeys[gal[s]]) for b, s in enumerate(sel)])

    def brk(self, dbrk, rset, dgks):
        k = B.MemBlindRotationEvaluationKeySet.__new__(B.MemBlindRotationEvaluationKeySet)
        k.BlindRotationKeys, k.AutomorphismKeys, k.rgsw, k.galois = dbrk, None, rset, dgks
        return k


@pytest.fixture(scope="module")
def edge(ctx):
    """edge(name, shape) -> one Edge per shape for this module's run (the rings and the oracle's tables are built once); the cache
    lives in the fixture, so every device object is released when the module is done"""
    cache = {}

    def make(name, s, **kw):
        if not kw and name in cache:
            return cache[name]
        S = Edge(ctx, s["logN"], s["q"], s["p"], s["pw2"], nj=s["nj"], **kw)
        if not kw:
            cache[name] = S
        return S

    yield make
    cache.clear()
    gc.collect()


def _check_select(S, ct, okeys, dset, sel=SEL):
    """out of place, the inputs unchanged, then in place: the oracle's words both times"""
    want = S.want_select(ct, okeys, sel)
    op0, out = S.up(ct), S.new_ct(len(sel))
    S.gev.AutomorphismSelect(op0, dset, sel, out)
    assert np.array_equal(S.down(out), want)
    assert np.array_equal(S.down(op0), ct), "the inputs were changed"
    S.gev.AutomorphismSelect(op0, dset, sel, op0)
    assert np.array_equal(S.down(op0), want)
    return want


def _check(S, seed, sel=SEL):
    rng = rng_for(seed)
    okeys, dset = S.galois(rng)
    assert len(okeys) >= 2
    return _check_select(S, S.cts(rng, len(sel)), okeys, dset, sel)


def _rc_select(S, op0, dset, sel, out):
    s = (C.c_int32 * len(sel))(*sel)
    return _lib.load().he_automorphism_ct_select(S.gev.h, op0[0].h, op0[1].h, dset.h, s, len(sel), out[0].h, out[1].h)


LIFT, INSIDE, OUTSIDE, MODULI = BE.lift_shapes(), BE.inside_shapes(), BE.outside_shapes(), BE.moduli_shapes()


# ---- A. the boundary of the copied ModDown's centred lift -----------------------------------------------------------------------------
@pytest.mark.parametrize("component", [0, 1])
@pytest.mark.parametrize("name", sorted(LIFT))
def test_lift_boundary(ctx, edge, name, component):
    """The coefficients of the P accumulator are planted -- (p - 1) / 2, (p + 1) / 2, 0 and p - 1 in turn, in one component
    (tests/test_blindrot_host.py holds that on the oracle) -- for the largest prime below 2^61, whose (p - 1) / 2 the reference's
    float quotient moves, a p below every Q limb and a p between two Q limbs.  in0 is uniform: the add and the permutation are in
    play.  Both keys of the set are planted ones."""
    S = edge(name, LIFT[name])
    rng = rng_for(10300 + component)
    okeys = {g: BE.planted_key(rng, S.oQ, S.oP, S.pw2, component) for g in BE.galois_pair(S.N)}
    ct = S.cts(rng, len(SEL))
    ct[:, 1] = R.ntt_of_one(S.oQ, S.level + 1)
    _check_select(S, ct, okeys, S.galois_set(okeys))


# ---- B. the edges of the domain -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(INSIDE))
def test_domain_edges_inside(ctx, edge, name):
    """the largest LDS footprint of each ring degree (64 KiB: 9x7, 10x3, 11x1), the last shift (63) and 255 windows"""
    s = INSIDE[name]
    assert BE.select_by_header(s)
    _check(edge(name, s), 10400)


@pytest.mark.parametrize("name", sorted(OUTSIDE))
def test_domain_edges_outside_are_einval(ctx, name):
    """one limb past each LDS bound, shift 64, two special primes, a conjugate-invariant ring: HE_EINVAL, nothing written"""
    s, ci = OUTSIDE[name]
    assert not BE.select_by_header(s, ci)
    S = Edge(ctx, s["logN"], s["q"], s["p"], s["pw2"], nj=s["nj"], ci=ci)
    rng = rng_for(10450)
    okeys, dset = S.galois(rng)
    ct = S.cts(rng, 2)
    op0, out = S.up(ct), S.up(ct ^ np.uint64(1))
    assert _rc_select(S, op0, dset, [0, 1], out) == EINVAL
    assert _rc_select(S, op0, dset, [1, -1], op0) == EINVAL
    assert np.array_equal(S.down(out), ct ^ np.uint64(1)) and np.array_equal(S.down(op0), ct)


def _core(S, rng, rows, n_keys=None, acc=None):
    """keys for every Galois element, n_keys RGSW keys, accumulators and the restatement's results"""
    rows = np.asarray(rows, dtype=np.uint64)
    ogks, dgks = S.galois(rng, BR.galois_elements(S.N))
    obrk, dbrk, rset = S.rgsw_set(rng, n_keys or rows.shape[1])
    acc = S.cts(rng, rows.shape[0]) if acc is None else acc
    want = np.stack([BR.blind_rotate_core(S.oev, rows[b], acc[b], obrk, ogks) for b in range(rows.shape[0])])
    return SimpleNamespace(BRK=S.brk(dbrk, rset, dgks), acc=acc, want=want, obrk=obrk, ogks=ogks)


def _profiled_core(S, ev, rows, acc, BRK):
    S.ctx.sync()
    S.ctx.prof_begin()
    try:
        ev.BlindRotateCore(rows, acc, BRK)
    finally:
        prof = S.ctx.prof_end()
    return prof


@pytest.mark.parametrize("name", ["10x4+P", "pw2-8-nj-9"])
def test_core_outside_the_select_domain_runs_per_entry(ctx, name):
    """he_blind_rotate_core still serves a shape the select forms refuse, entry by entry: no automorphism_ct_select launch"""
    s, _ = OUTSIDE[name]
    S = Edge(ctx, s["logN"], s["q"], s["p"], s["pw2"], nj=s["nj"])
    rng = rng_for(10480)
    g = lambda k: pow(5, k, 2 * S.N)
    rows = np.array([[g(3), 0, 2 * S.N - g(7)], [g(S.N // 2 - 1), g(3), 1]], dtype=np.uint64)
    c = _core(S, rng, rows)
    acc = S.up(c.acc)
    prof = _profiled_core(S, B.Evaluator(S.gev._ev, S.gQ), rows, acc, c.BRK)
    assert prof and K_AUTO not in prof, prof
    assert np.array_equal(S.down(acc), c.want)


# ---- C. keys below the evaluator's top level, limbs above the keys' --------------------------------------------------------------------
@pytest.fixture(scope="module")
def c_moduli():
    return E.moduli(10, (35, 20, 45, 27), (61,))


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("level", [0, 1, 2])
def test_keys_below_the_top_level(ctx, c_moduli, level, inplace):
    """one evaluator (four Q limbs, one special prime): the special prime's modulus record is the evaluator's (index 4) and its
    limb inside a key block the key's (level + 1); polynomials of four limbs keep the words of the limbs above the keys' level on
    working and on pass-through entries"""
    q, p = c_moduli
    S = Edge(ctx, 10, q, p, 7, level=level)
    rng = rng_for(10500 + level)
    okeys, dset = S.galois(rng)
    assert all(k.LevelQ() == level for k in okeys.values()) and len(S.q) == 4
    ct = S.cts(rng, len(SEL))
    got = _run_at_level(S, None, dset, ct, lambda a, k, o: S.gev.AutomorphismSelect(a, k, SEL, o), inplace)
    assert np.array_equal(got, S.want_select(ct, okeys, SEL))


def test_keys_at_the_top_level_are_outside_the_domain(ctx, c_moduli):
    q, p = c_moduli
    S = Edge(ctx, 10, q, p, 7, level=3)
    rng = rng_for(10540)
    okeys, dset = S.galois(rng)
    ct = S.cts(rng, 2)
    op0, out = S.up(ct), S.up(ct ^ np.uint64(1))
    assert _rc_select(S, op0, dset, [0, 1], out) == EINVAL
    assert np.array_equal(S.down(out), ct ^ np.uint64(1)) and np.array_equal(S.down(op0), ct)


def test_core_with_keys_below_the_top_level(ctx, c_moduli):
    """level-1 keys on four-limb accumulators, one row all zero: the batched route, limbs 2 and 3 untouched"""
    q, p = c_moduli
    S = Edge(ctx, 10, q, p, 7, level=1)
    rng = rng_for(10550)
    g = lambda k: pow(5, k, 2 * S.N)
    rows = np.array([[g(12), 2 * S.N - g(5), g(12)], [0, 0, 0], [2 * S.N - 1, g(1), g(S.N // 2 - 1)]], dtype=np.uint64)
    c = _core(S, rng, rows)
    acc = S.up(c.acc, nlimbs=4)
    prof = _profiled_core(S, B.Evaluator(S.gev._ev, S.gQ), rows, acc, c.BRK)
    assert prof[K_AUTO][0] >= 1 and prof[K_PROD][0] >= 1 and set(prof) == {K_AUTO, K_PROD}, prof
    for k in range(2):
        assert np.array_equal(acc[k].download()[:, 2:], np.full((3, 2, S.N), 0x5A5A, dtype=np.uint64)), k
    assert np.array_equal(S.down(acc), c.want)


# ---- D. moduli ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODULI))
def test_moduli_at_the_class_boundaries(ctx, edge, name):
    """primes next to 2^47, 2^58 and 2^61 as sources, destinations and special primes; the 14-bit prime as a destination below a
    14-bit and a 16-bit window's mask (reduced before its transform: the only such limb of its chain) and above a 13-bit one's"""
    s = MODULI[name]
    S = edge(name, s)
    if "pw2-14" in name or "pw2-16" in name:
        assert [((1 << s["pw2"]) - 1) >= m for m in s["q"] + s["p"]].count(True) == 1
    _check(S, 10600)


# ---- E. words -------------------------------------------------------------------------------------------------------------------------
WORD_SHAPES = {**INSIDE, **MODULI}
LAZY_KINDS = ("max_lazy", "alt_lazy", "uniform_lazy", "max", "uniform")


@pytest.mark.parametrize("name", sorted(WORD_SHAPES))
def test_worst_case_words(ctx, edge, name):
    """eleven entries: in1 walks through max, alt, alt_lazy, half, max_lazy, uniform_lazy (words up to 2q - 1) and the
    coefficient-domain worst cases NTT(all q - 1), NTT(every window = mask), NTT(0); in0 through the lazy kinds -- the reference
    adds it with ONE conditional subtraction, so words at or above q come out and the device returns those very words; the key
    rows walk through the canonical kinds"""
    s = WORD_SHAPES[name]
    base = edge(name, s)
    S = edge(name, s, key_words=Bd.WordCycle(Bd.CANONICAL_KINDS, start=1), in0_words=Bd.WordCycle(LAZY_KINDS, start=len(name)),
             in1_words=E.CtCycle(base.oQ, s["pw2"], start=len(name)))
    sel = [0, 1, 1, 0, 0, 1, 0, 1, 1, -1, 0]  # (nine working entries first: in1 meets every kind of the cycle)
    want = _check(S, 10700, sel)
    top = max(int((want[b, 0, u] // np.uint64(m)).max()) for b, x in enumerate(sel) if x >= 0 for u, m in enumerate(S.q[: S.level + 1]))
    assert top == 1, "no word of the oracle's component 0 reached q"


# ---- F. lazy key words on Galois keys ---------------------------------------------------------------------------------------------------
def _lazy_galois(S, rng):
    """two Galois keys after AddLazy (M = 2): words below 2q on the device and in the oracle's keys"""
    oA, oB = [[S.okey(rng) for _ in range(2)] for _ in range(2)]
    dA, dB = [G.Ciphertext(S.dkey(o[0]), S.dkey(o[1])) for o in (oA, oB)]
    G.AddLazy(dA, None, dB)
    oB = R.add_lazy_ciphertext(S.oQ, S.oP, oA, oB)
    top = max(int((k.q[:, :, u] // np.uint64(m)).max()) for k in oB for u, m in enumerate(S.q[: S.level + 1]))
    assert top == 1, "no key word reached q"
    g = BE.galois_pair(S.N)
    return oB, dB, B.GaloisKeySet(S.gev._ev, {g[0]: dB.Value[0], g[1]: dB.Value[1]})


def test_lazy_key_words_are_served_where_the_reference_is_exact(ctx):
    q, p = E.moduli(10, (35, 20), (55,))
    S = Edge(ctx, 10, q, p, 7)
    rng = rng_for(10800)
    oB, dB, dset = _lazy_galois(S, rng)
    assert R.key_words_in_domain(S.oQ, S.oP, oB, 2)
    g = BE.galois_pair(S.N)
    _check_select(S, S.cts(rng, len(SEL)), {g[0]: oB[0], g[1]: oB[1]}, dset)


def test_lazy_key_words_are_refused_where_the_reference_leaves_its_domain(ctx):
    """a 61-bit special prime leaves no room for M = 2: HE_EINVAL naming HE_RGSW_REDUCE, nothing written; served after Reduce"""
    q, p = E.moduli(10, (35, 20), (61,))
    S = Edge(ctx, 10, q, p, 7)
    rng = rng_for(10850)
    oB, dB, dset = _lazy_galois(S, rng)
    assert R.key_words_in_domain(S.oQ, S.oP, oB, 1) and not R.key_words_in_domain(S.oQ, S.oP, oB, 2)
    ct = S.cts(rng, len(SEL))
    op0, out = S.up(ct), S.up(ct ^ np.uint64(1))
    with pytest.raises(la.HeringError) as e:
        B.AutomorphismSelect(S.gev._ev, op0, dset, SEL, out)
    assert e.value.code == EINVAL and "REDUCE" in str(e.value)
    assert np.array_equal(S.down(out), ct ^ np.uint64(1)) and np.array_equal(S.down(op0), ct)
    G.Reduce(dB, None, dB)
    oB = R.reduce(S.oQ, S.oP, oB, oB)
    g = BE.galois_pair(S.N)
    _check_select(S, ct, {g[0]: oB[0], g[1]: oB[1]}, dset)


# ---- G. the select form beyond one fill of the selection --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def select_case(ctx):
    """logN 9, one 14-bit limb, two windows; three keys, three ciphertexts and their nine automorphisms"""
    S = Edge(ctx, 9, [E.Q14], [], 7)
    rng = rng_for(10900)
    gal = BR.galois_elements(S.N)
    okeys, dset = S.galois(rng, [gal[0], gal[10], gal[9]])
    cts = S.cts(rng, 3)
    autos = np.stack([np.stack([S.oev.Automorphism(cts[i], g, k) for i in range(3)]) for g, k in okeys.items()])  # [key][ct]
    return S, dset, cts, autos


@pytest.mark.parametrize("B_", [895, 896, 897])
def test_select_beyond_one_fill(ctx, select_case, B_):
    """896 entries are one fill of the selection (448 words of two entries); 895 ends in half a word, 897 takes a second fill"""
    S, dset, cts, autos = select_case
    which, sel = _select_batch(B_)
    assert set(sel.tolist()) == {-1, 0, 1, 2} and (B_ + 1) // 2 <= BE.FILL_WORDS + (B_ > 896)
    ct = cts[which]
    want = np.where((sel < 0)[:, None, None, None], ct, autos[np.maximum(sel, 0), which])
    op0, out = S.up(ct), S.new_ct(B_)
    S.gev.AutomorphismSelect(op0, dset, sel, out)
    assert np.array_equal(S.down(out), want)
    assert np.array_equal(S.down(op0), ct)
    S.gev.AutomorphismSelect(op0, dset, sel, op0)
    assert np.array_equal(S.down(op0), want)


def test_select_all_entries_pass_through(ctx, select_case):
    S, dset, cts, autos = select_case
    which, sel = _select_batch(7, all_pass=True)
    ct = cts[which]
    op0, out = S.up(ct), S.new_ct(7)
    S.gev.AutomorphismSelect(op0, dset, sel, out)
    assert np.array_equal(S.down(out), ct) and np.array_equal(S.down(op0), ct)
    S.gev.AutomorphismSelect(op0, dset, sel, op0)
    assert np.array_equal(S.down(op0), ct)


# ---- H. schedule edges of the batched core ----------------------------------------------------------------------------------------------
class RowCase:
    """logN 9, [Q27], no special prime, pw2 7, sixteen RGSW keys: the rows of tests/blindrot_edges.rows(), one accumulator per row
    (rows 0-2 share theirs) and the restatement's result of each, computed once"""

    def __init__(self, ctx):
        self.S = S = Edge(ctx, BE.ROW_LOGN, [BE.Q27], [], 7)
        rng = rng_for(11000)
        self.rows = BE.rows()
        acc = S.cts(rng, len(self.rows))
        acc[1] = acc[2] = acc[0]
        c = _core(S, rng, self.rows, acc=acc)
        self.BRK, self.acc, self.want, self.obrk, self.ogks = c.BRK, c.acc, c.want, c.obrk, c.ogks
        self.ev = B.Evaluator(S.gev._ev, S.gQ)

    def batch(self, idx):
        return self.rows[idx], self.acc[idx], self.want[idx]


@pytest.fixture(scope="module")
def rowcase(ctx):
    return RowCase(ctx)


def _census(rounds):
    return sum(1 for g, _ in rounds if np.any(g != 0)), sum(1 for _, p in rounds if np.any(p >= 0))


@pytest.mark.parametrize("B_", [10, 7, 14, 11])
def test_core_schedule_edges(ctx, rowcase, B_):
    """ten rows in one batch (all 0 / 1 / 2N - 1, the first and last step of either walk, sets on and beside the window's flush,
    random): entries idle for many rounds while others work.  B = 7 takes a second fill of the selection table, B = 14 a third
    (tests/test_blindrot_host.py holds the sizes); B = 11 adds our negative-walk row.  The launch census is the non-empty rounds."""
    c = rowcase
    idx = BE.batch_of(B_) if B_ != 11 else list(range(11))
    rows, start, want = c.batch(idx)
    rounds = B.Rounds(c.S.logN, rows)
    words = (2 * len(rounds) * B_ + 1) // 2
    assert words > BE.FILL_WORDS and (words > 2 * BE.FILL_WORDS) == (B_ >= 14)
    acc = c.S.up(start)
    c.ev.BlindRotateCore(rows, acc, c.BRK)  # (the scratch arena is sized on first use)
    assert np.array_equal(c.S.down(acc), want)
    acc = c.S.up(start)
    prof = _profiled_core(c.S, c.ev, rows, acc, c.BRK)
    n_auto, n_prod = _census(rounds)
    assert prof[K_AUTO][0] == n_auto and prof[K_PROD][0] == n_prod and sum(n for n, _ in prof.values()) == n_auto + n_prod, prof
    got = c.S.down(acc)
    assert np.array_equal(got, want)
    if B_ >= 10:
        assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2]), "0, 1 and 2N - 1 share set 0"


def test_core_schedule_edges_one_fill(ctx, rowcase):
    """B = 5 (rows 0-4): the table fits one fill"""
    c = rowcase
    rows, start, want = c.batch(list(range(5)))
    assert (2 * len(B.Rounds(c.S.logN, rows)) * 5 + 1) // 2 <= BE.FILL_WORDS
    acc = c.S.up(start)
    c.ev.BlindRotateCore(rows, acc, c.BRK)
    assert np.array_equal(c.S.down(acc), want)


@pytest.mark.parametrize("mode", ["graph", "replay"])
def test_core_three_fills_call_modes(ctx, rowcase, mode):
    """B = 14 under graph capture with two replays, and through trace / replay once: the three fills are frozen with the call"""
    c = rowcase
    rows, start, want = c.batch(BE.batch_of(14))
    acc = c.S.up(start)
    c.ev.BlindRotateCore(rows, acc, c.BRK)  # (sizes the scratch arena)
    ctx.sync()
    fresh = c.S.up(start)
    reset = lambda: [a.CopyLvl(c.S.level, s) for a, s in zip(acc, fresh)]
    reset()
    ctx.sync()
    if mode == "graph":
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


@pytest.mark.parametrize("n_lwe", [1, 5])
def test_core_fewer_words_than_keys(ctx, rowcase, n_lwe):
    """n_lwe = 1, and n_lwe smaller than the RGSW set of sixteen: rows 0, 5, 7, 9 cut to their first n_lwe words"""
    c = rowcase
    idx = [0, 5, 7, 9]
    rows = np.ascontiguousarray(c.rows[idx][:, :n_lwe])
    start = c.acc[idx]
    want = np.stack([BR.blind_rotate_core(c.S.oev, rows[b], start[b], c.obrk, c.ogks) for b in range(len(idx))])
    acc = c.S.up(start)
    c.ev.BlindRotateCore(rows, acc, c.BRK)
    assert np.array_equal(c.S.down(acc), want)
    assert n_lwe < len(c.BRK.BlindRotationKeys) == BE.ROW_N_LWE


# ---- I. operand identity ----------------------------------------------------------------------------------------------------------------
def test_operand_identity_select(ctx):
    row = BA.ROWS["he_automorphism_ct_select"]
    q, p = E.moduli(10, (35, 20), (61,))
    S = Edge(ctx, 10, q, p, 7)
    rng = rng_for(11200)
    okeys, dset = S.galois(rng)
    gal = list(okeys)
    L = _lib.load()
    sel = (C.c_int32 * 1)(1)
    names = list(row.params)
    for a, b in itertools.combinations(names, 2):
        words = {n: uniform_poly(rng, S.q, S.N)[None] for n in names}
        polys = {n: la.Poly(S.gQ, S.level + 1, 1).upload(words[n]) for n in names}
        polys[b] = polys[a]
        words[b] = words[a]
        rc = L.he_automorphism_ct_select(S.gev.h, polys["in0"].h, polys["in1"].h, dset.h, sel, 1, polys["out0"].h, polys["out1"].h)
        got = {n: polys[n].download() for n in names}
        if row.verdict(a, b) == "reject":
            assert rc == EINVAL, (a, b)
            for n in names:
                assert np.array_equal(got[n], words[n]), (a, b, n)
        else:
            assert rc == 0, (a, b, L.he_last_error())
            want = S.oev.Automorphism(np.stack([words["in0"][0], words["in1"][0]]), gal[1], okeys[gal[1]])
            assert np.array_equal(got["out0"][0], want[0]) and np.array_equal(got["out1"][0], want[1]), (a, b)


def test_operand_identity_core(ctx, rowcase):
    row = BA.ROWS["he_blind_rotate_core"]
    assert list(row.params) == ["acc0", "acc1"] and row.verdict("acc0", "acc1") == "reject"
    c = rowcase
    rows, start, want = c.batch([9])
    acc = c.S.up(start)
    L = _lib.load()
    r = np.ascontiguousarray(rows)
    for one in (acc[0], acc[1]):
        assert L.he_blind_rotate_core(c.S.gev.h, r.ctypes.data_as(_lib.u64p), 1, BE.ROW_N_LWE, one.h, one.h, c.BRK.rgsw.h, c.BRK.galois.h) == EINVAL
    assert np.array_equal(c.S.down(acc), start), "a rejection wrote something"
    assert L.he_blind_rotate_core(c.S.gev.h, r.ctypes.data_as(_lib.u64p), 1, BE.ROW_N_LWE, acc[0].h, acc[1].h, c.BRK.rgsw.h, c.BRK.galois.h) == 0
    assert np.array_equal(c.S.down(acc), want)
