"""The RGSW external product at the edges of its domain, words and moduli (include/hering_rgsw.h), word for word against
tests/rgsw_ref.py on the oracle.  tests/test_gpu_rgsw.py holds the product with uniformly random canonical words at a few
shapes; this file plants the values and builds the shapes at which the one-launch kernel, its dispatch and the generic route
can be wrong without those tests noticing (tests/rgsw_edges.py builds them, tests/test_rgsw_host.py checks without a device that
each has the property it is built for).  Every case that claims a route asserts it from the launch profile before any word is
compared: the one-launch route is one launch of "rgsw_external_product", the generic route none."""
import ctypes as C
import gc

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd import _lib
from lattigo_amd import rgsw as G
from tests import boundary as Bd
from tests import rgsw_edges as E
from tests import rgsw_ref as R
from tests.gpu_common import ctx  # noqa: F401
from tests.helpers import rng_for, uniform_poly
from tests.test_gpu_rgsw import EINVAL, KERNEL, Setup, _check

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_garbage_left_behind():
    gc.collect()
    yield
    gc.collect()


class Routed:
    """rgsw.Evaluator whose products assert the route they took from the launch profile"""

    def __init__(self, ev, ctx, route):
        self._ev, self._ctx, self.route, self.prof = ev, ctx, route, None

    def __getattr__(self, name):
        if name.startswith("_"):  # (never forward a lookup of the wrapper's own fields: it would recurse)
            raise AttributeError(name)
        return getattr(self._ev, name)

    def _profiled(self, call, route):
        self._ctx.sync()
        self._ctx.prof_begin()
        try:
            call()
        finally:
            self.prof = self._ctx.prof_end()
        if route == E.ONE:
            assert KERNEL in self.prof and self.prof[KERNEL][0] == 1, self.prof
        elif route == E.GEN:
            assert KERNEL not in self.prof and self.prof, self.prof

    def ExternalProduct(self, op0, op1, opOut):
        self._profiled(lambda: self._ev.ExternalProduct(op0, op1, opOut), self.route)

    def ExternalProductSelect(self, op0, keys, sel, opOut):
        self._profiled(lambda: self._ev.ExternalProductSelect(op0, keys, sel, opOut), E.ONE)


class Edge(Setup):
    """Setup with keys below the ring's top level, chosen window counts, other word sources and the route assertion"""

    def __init__(self, ctx, logN, q, p, pw2, route, nj=None, level=None, key_words=None, ct_words=None):
        super().__init__(ctx, logN, q, p, pw2)
        self.gev = Routed(self.gev, ctx, route)
        self.nj, self.key_words, self.ct_words = nj, key_words, ct_words
        if level is not None:
            self.level = level

    def device(self, o):
        kw = dict(BaseTwoDecomposition=self.pw2, BaseTwoDecompositionVectorSize=o[0].nj) if self.pw2 else {}
        return self.gev.NewCiphertext(o[0].q, o[0].p if self.p else None, o[1].q, o[1].p if self.p else None, **kw)

    def rgsw(self, rng):
        o = R.uniform_rgsw(rng, self.oQ, self.oP, self.pw2, levelQ=self.level, nj=self.nj, words=self.key_words)
        return o, self.device(o)

    def cts(self, rng, batch):
        src = self.ct_words or uniform_poly
        mods = self.q[: self.level + 1]
        return np.stack([np.stack([src(rng, mods, self.N) for _ in range(2)]) for _ in range(batch)])


@pytest.fixture(scope="module")
def edge(ctx):
    """edge(name, shape) -> one Edge per shape for this module's run (the rings and the oracle's tables are built once); the cache
    lives in the fixture, so every device object is released when the module is done and none waits for the interpreter's exit"""
    cache = {}

    def make(name, s, **kw):
        if not kw and name in cache:
            return cache[name]
        S = Edge(ctx, s["logN"], s["q"], s["p"], s["pw2"], s["route"], nj=s["nj"], **kw)
        if not kw:
            cache[name] = S
        return S

    yield make
    cache.clear()
    gc.collect()


DOMAIN, SHIFT, MODULI, LIFT, DIGITS = E.domain_shapes(), E.shift_shapes(), E.moduli_shapes(), E.lift_shapes(), E.digit_index_shapes()


# ---- A. the boundary of ModDown's centred lift ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("component", [0, 1])
@pytest.mark.parametrize("name", sorted(LIFT))
def test_lift_boundary(ctx, edge, name, component):
    """The coefficients of the P accumulator are planted: (p - 1) / 2 (the last residue that is not moved), (p + 1) / 2 (the first
    that is), 0 and p - 1, in turn, in one output component.  p: the largest prime below 2^61; a p below every Q limb (p mod q = p);
    a p between two Q limbs."""
    S = edge(name, LIFT[name])
    rng = rng_for(9400 + component)
    okeys = R.planted_rgsw(rng, S.oQ, S.oP, S.pw2, component)
    ct = np.stack([R.ntt_of_one(S.oQ, S.level + 1), np.zeros((S.level + 1, S.N), dtype=np.uint64)])[None]
    want, pc = R.external_product(S.oev, ct[0], okeys, with_p_coeffs=True)
    assert np.array_equal(pc[component, 0], R.lift_targets(S.p[0], S.N)) and not pc[1 - component].any()
    op0, out = S.up(ct), S.new_ct(1)
    S.gev.ExternalProduct(op0, S.device(okeys), out)
    assert np.array_equal(S.down(out)[0], want)


# ---- B. the edges of the one-launch domain -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("name", sorted(DOMAIN))
def test_domain_edges(ctx, edge, name, inplace):
    """the largest LDS footprint of each ring degree and the first shape outside it"""
    s = DOMAIN[name]
    assert (s["route"] == E.ONE) == E.fused_by_header(s["logN"], len(s["q"]), len(s["p"]))
    _check(edge(name, s), 9500 + inplace, 2, inplace)


@pytest.mark.parametrize("name", sorted(SHIFT))
def test_window_shift_bound(ctx, edge, name):
    """(nj - 1) pw2 = 63 is the last shift of the one-launch kernel; at 64 the generic route serves a window of zero"""
    s = SHIFT[name]
    assert ((s["nj"][0] - 1) * s["pw2"] < 64) == (s["route"] == E.ONE) and (s["nj"][0] - 1) * s["pw2"] in (63, 64)
    S = edge(name, s)
    _check(S, 9520, 2)
    _check(S, 9521, 1, inplace=True)


def test_digit_index_255_windows(ctx, edge):
    """255 windows, the most a key takes: digit indices up to 254 through the kernel's uint8_t prefix[] on the one-launch route"""
    S = edge("beta255", DIGITS["beta255"])
    orgsw, _, _, _ = _check(S, 9530, 1)
    assert orgsw[0].q.shape[0] == 255


@pytest.mark.parametrize("name", ["prefix255", "prefix256"])
def test_digit_index_256_is_not_a_key(ctx, name):
    """a shape whose last limb starts at digit 255 or beyond has 256 or more windows: he_evk_create_base2 refuses the key, so no
    product -- on either route -- meets a digit index that does not fit uint8_t"""
    s = DIGITS[name]
    S = Edge(ctx, s["logN"], s["q"], s["p"], s["pw2"], None)
    o = R.uniform_rgsw(rng_for(9540), S.oQ, S.oP, S.pw2)
    assert sum(o[0].nj[:-1]) >= 255
    with pytest.raises(la.HeringError) as e:
        S.device(o)
    assert e.value.code == EINVAL and "255" in str(e.value)


# ---- C. keys below the evaluator's top level -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c_moduli():
    return E.moduli(10, (35, 20, 45, 27), (61,))


def _above(B, n, N, word):
    return np.full((B, n, N), word, dtype=np.uint64)


def _run_at_level(S, orgsw, dkeys, ct, call, inplace):
    """polynomials of all the ring's limbs: limbs above the keys' level keep their words (0x5A5A.. in, 0x77 out)"""
    B, top = ct.shape[0], len(S.q)
    op0 = S.up(ct, nlimbs=top)
    out = op0 if inplace else [la.Poly(S.gQ, top, B).upload(np.concatenate([ct[:, k] ^ np.uint64(1), _above(B, top - S.level - 1, S.N, 0x77)], axis=1))
                               for k in range(2)]
    call(op0, dkeys, out)
    for k in range(2):
        got = out[k].download()
        assert np.array_equal(got[:, S.level + 1:], _above(B, top - S.level - 1, S.N, 0x5A5A if inplace else 0x77)), k
    return np.stack([o.download()[:, : S.level + 1] for o in out], axis=1)


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("pw2", [7, 0])
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_keys_below_the_top_level(ctx, c_moduli, level, pw2, inplace):
    """one evaluator (four Q limbs, one special prime) takes both routes: the route follows the key's level, the special prime's
    modulus record is the evaluator's (LQ) and its limb inside a key block the key's (nQk)"""
    q, p = c_moduli
    S = Edge(ctx, 10, q, p, pw2, E.ONE if level < 3 else E.GEN, level=level)
    rng = rng_for(9600 + 10 * level + pw2)
    orgsw, dkeys = S.rgsw(rng)
    assert orgsw[0].LevelQ() == level and dkeys.LevelQ() == level
    ct = S.cts(rng, 2)
    got = _run_at_level(S, orgsw, dkeys, ct, S.gev.ExternalProduct, inplace)
    assert np.array_equal(got, S.want(ct, orgsw))


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
def test_select_below_the_top_level(ctx, c_moduli, inplace):
    q, p = c_moduli
    S = Edge(ctx, 10, q, p, 7, E.ONE, level=1)
    rng = rng_for(9650)
    keys = [S.rgsw(rng) for _ in range(2)]
    dset = S.gev.NewKeySet([k[1] for k in keys])
    sel = [1, -1, 0]
    ct = S.cts(rng, 3)
    want = np.stack([ct[b] if s < 0 else R.external_product(S.oev, ct[b], keys[s][0]) for b, s in enumerate(sel)])
    got = _run_at_level(S, None, dset, ct, lambda a, k, o: S.gev.ExternalProductSelect(a, k, sel, o), inplace)
    assert np.array_equal(got, want)


# ---- D. moduli -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODULI))
def test_moduli_at_the_class_boundaries(ctx, edge, name):
    """primes next to 2^47, 2^58 and 2^61 as sources, destinations and special primes on both routes; the 14-bit prime as a
    destination below a 14-bit window's mask (reduced first: the only such limb of its chain) and above a 13-bit one's"""
    s = MODULI[name]
    S = edge(name, s)
    if "pw2-14" in name:
        assert [((1 << s["pw2"]) - 1) >= m for m in s["q"] + s["p"]].count(True) == 1
    _check(S, 9700, 2)
    _check(S, 9701, 1, inplace=True)


# ---- E. words --------------------------------------------------------------------------------------------------------------------
WORD_SHAPES = {**DOMAIN, **MODULI}


@pytest.mark.parametrize("name", sorted(WORD_SHAPES))
def test_worst_case_words(ctx, edge, name):
    """five entries = ten polynomials walk through max, alt, alt_lazy, half, max_lazy, uniform_lazy (words up to 2q - 1) and the
    coefficient-domain worst cases NTT(all q - 1), NTT(every window = mask), NTT(0); the key rows walk through the canonical kinds"""
    s = WORD_SHAPES[name]
    base = edge(name, s)
    S = edge(name, s, key_words=Bd.WordCycle(Bd.CANONICAL_KINDS, start=1), ct_words=E.CtCycle(base.oQ, s["pw2"], start=len(name)))
    _check(S, 9800, 5)
    S.ct_words = E.CtCycle(base.oQ, s["pw2"], start=len(name) + 3)
    _check(S, 9801, 2, inplace=True)


# ---- F. key words at or above q --------------------------------------------------------------------------------------------------
def _lazy_key(S, rng, doubled_max=False):
    """B += A without reduction: words below 2q on the device and in the oracle's keys.  doubled_max: A of `max` rows added to
    itself, every word 2q - 2 -- the top of the bound M = 2, where uniform keys only meet its interior"""
    if doubled_max:
        S.key_words = Bd.WordCycle(("max",))
        oB, dB = S.rgsw(rng)
        S.key_words = None
        G.AddLazy(dB, None, dB)
        oB = R.add_lazy_ciphertext(S.oQ, S.oP, oB, oB)
        assert all(int(k.q[:, :, u].min()) == 2 * m - 2 for k in oB for u, m in enumerate(S.q[: S.level + 1]))
        return oB, dB
    oA, dA = S.rgsw(rng)
    oB, dB = S.rgsw(rng)
    G.AddLazy(dA, None, dB)
    oB = R.add_lazy_ciphertext(S.oQ, S.oP, oA, oB)
    top = max(int((k.q[:, :, u] // np.uint64(m)).max()) for k in oB for u, m in enumerate(S.q[: S.level + 1]))
    assert top == 1, "no key word reached q"
    return oB, dB


@pytest.mark.parametrize("doubled_max", [False, True], ids=["uniform-sum", "max-doubled"])
@pytest.mark.parametrize("case", ["one-launch", "one-launch-no-P", "one-launch-32bit", "generic", "generic-branch-M"])
def test_lazy_key_words_are_served_where_the_reference_is_exact(ctx, case, doubled_max):
    """hering_rgsw.h, "Key words": a key after AddLazy (M = 2) is served with the reference's words while
    (M q - 1)(6q - 2) < q 2^64 (bit windows), (M q - 1)(2q - 1) < q 2^64 (branch M), 2 D W (M q - 1) < 2^64 (32-bit branch)"""
    logq, logp, pw2, route = {"one-launch": ((35, 20), (55,), 7, E.ONE), "one-launch-no-P": ((35, 60), (), 13, E.ONE),
                              "one-launch-32bit": ((27,), (), 7, E.ONE), "generic": ((35, 20, 45, 60), (58,), 13, E.GEN),
                              "generic-branch-M": ((35, 20), (55, 60), 0, E.GEN)}[case]
    q, p = E.moduli(10, logq, logp)
    S = Edge(ctx, 10, q, p, pw2, route)
    rng = rng_for(9900 + len(case))
    okey, dkey = _lazy_key(S, rng, doubled_max)
    assert R.key_words_in_domain(S.oQ, S.oP, okey, 2)
    ct = S.cts(rng, 2)
    op0, out = S.up(ct), S.new_ct(2)
    S.gev.ExternalProduct(op0, dkey, out)
    assert np.array_equal(S.down(out), S.want(ct, okey))
    if route == E.ONE:
        dset = S.gev.NewKeySet([dkey])
        out2 = S.new_ct(2)
        S.gev.ExternalProductSelect(op0, dset, [0, 0], out2)
        assert np.array_equal(S.down(out2), S.want(ct, okey))


@pytest.mark.parametrize("case", ["one-launch", "generic", "32bit"])
def test_lazy_key_words_are_refused_where_the_reference_leaves_its_domain(ctx, case):
    """a 61-bit modulus leaves no room for M = 2 ((2q - 1)(6q - 2) >= q 2^64); the 32-bit branch's sum at q ~ 2^28.5 and eight
    windows holds canonical keys only.  The call is HE_EINVAL, nothing is written, and the product is served after Reduce."""
    logq, logp, pw2, route = {"one-launch": ((35, 20), (61,), 7, E.ONE), "generic": ((35, 20, 45, 27), (61,), 7, E.GEN),
                              "32bit": (None, (), 4, E.ONE)}[case]
    q, p = ([E.wrap_primes()[0]], []) if logq is None else E.moduli(10, logq, logp)
    S = Edge(ctx, 10, q, p, pw2, route)
    rng = rng_for(9950 + len(case))
    okey, dkey = _lazy_key(S, rng)
    assert R.key_words_in_domain(S.oQ, S.oP, okey, 1) and not R.key_words_in_domain(S.oQ, S.oP, okey, 2)
    ct = S.cts(rng, 1)
    op0, out = S.up(ct), S.up(ct ^ np.uint64(1))
    with pytest.raises(la.HeringError) as e:
        S.gev._ev.ExternalProduct(op0, dkey, out)
    assert e.value.code == EINVAL and "REDUCE" in str(e.value)
    if route == E.ONE:
        dset = S.gev.NewKeySet([dkey])
        with pytest.raises(la.HeringError) as e:
            S.gev._ev.ExternalProductSelect(op0, dset, [0], out)
        assert e.value.code == EINVAL
    assert np.array_equal(S.down(out), ct ^ np.uint64(1)) and np.array_equal(S.down(op0), ct)
    G.Reduce(dkey, None, dkey)
    okey = R.reduce(S.oQ, S.oP, okey, okey)
    S.gev.ExternalProduct(op0, dkey, out)
    assert np.array_equal(S.down(out), S.want(ct, okey))


def test_lazy_key_bound_is_not_kept_beyond_2_pow_32(ctx):
    """AddLazy(k, k) doubles the bound M; past 2^32 it is no longer kept (the words themselves wrap 2^64 a little later) and
    the key is refused, however small the modulus, until it is reduced"""
    S = Edge(ctx, 9, [E.Q14], [], 7, E.ONE)
    rng = rng_for(9990)
    okey, dkey = S.rgsw(rng)
    ct = S.cts(rng, 1)
    op0, out = S.up(ct), S.up(ct ^ np.uint64(1))
    for n in range(1, 34):
        G.AddLazy(dkey, None, dkey)
        okey = R.add_lazy_ciphertext(S.oQ, S.oP, okey, okey)
        if n == 20:  # M = 2^20: 2 D W (M q - 1) = 2 * 2 * 6q * 2^20 q ~ 2^52, served
            assert R.key_words_in_domain(S.oQ, S.oP, okey, 1 << 20)
            S.gev.ExternalProduct(op0, dkey, out)
            assert np.array_equal(S.down(out), S.want(ct, okey))
            out = S.up(ct ^ np.uint64(1))
    with pytest.raises(la.HeringError) as e:
        S.gev._ev.ExternalProduct(op0, dkey, out)
    assert e.value.code == EINVAL and "REDUCE" in str(e.value)
    assert np.array_equal(S.down(out), ct ^ np.uint64(1))
    G.Reduce(dkey, None, dkey)
    S.gev.ExternalProduct(op0, dkey, out)
    assert np.array_equal(S.down(out), S.want(ct, R.reduce(S.oQ, S.oP, okey, okey)))


# ---- G. the select form beyond one fill of the selection -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def select_case(ctx):
    """logN 9, one 14-bit limb, two windows; three keys, three ciphertexts and their nine products"""
    S = Edge(ctx, 9, [E.Q14], [], 7, E.ONE)
    rng = rng_for(10000)
    keys = [S.rgsw(rng) for _ in range(3)]
    assert keys[0][0][0].q.shape[0] == 2
    cts = S.cts(rng, 3)
    prods = np.stack([np.stack([R.external_product(S.oev, cts[i], k[0]) for i in range(3)]) for k in keys])  # [key][ct]
    return S, keys, S.gev.NewKeySet([k[1] for k in keys]), cts, prods


def _select_batch(B, all_pass=False):
    """entry b: ciphertext b mod 3, key (b div 3) mod 4 - 1: every (ciphertext, key or -1) pair; an odd batch ends in -1"""
    which = np.arange(B) % 3
    sel = ((np.arange(B) // 3) % 4 - 1).astype(np.int32)
    if all_pass:
        sel[:] = -1
    elif B & 1:
        sel[-1] = -1
    return which, sel


@pytest.mark.parametrize("B", [895, 896, 897, 1793])
def test_select_beyond_one_fill(ctx, select_case, B):
    """896 entries are one fill of the selection (448 words of two entries); 895 ends in half a word, 897 and 1793 take a second
    and a third fill.  The fill is not a profiled kernel: the chunks are held by the words of every entry."""
    S, keys, dset, cts, prods = select_case
    which, sel = _select_batch(B)
    assert set(sel.tolist()) == {-1, 0, 1, 2} and (B % 2 == 0 or sel[-1] == -1)
    ct = cts[which]
    want = np.where((sel < 0)[:, None, None, None], ct, prods[np.maximum(sel, 0), which])
    op0, out = S.up(ct), S.new_ct(B)
    S.gev.ExternalProductSelect(op0, dset, sel, out)
    assert set(S.gev.prof) == {KERNEL}, S.gev.prof  # (the fills are not profiled: the kernel's one launch is the whole profile)
    assert np.array_equal(S.down(out), want)
    S.gev.ExternalProductSelect(op0, dset, sel, op0)
    assert np.array_equal(S.down(op0), want)


def test_select_all_entries_pass_through(ctx, select_case):
    S, keys, dset, cts, prods = select_case
    which, sel = _select_batch(7, all_pass=True)
    ct = cts[which]
    op0, out = S.up(ct), S.new_ct(7)
    S.gev.ExternalProductSelect(op0, dset, sel, out)
    assert np.array_equal(S.down(out), ct) and np.array_equal(S.down(op0), ct)
    S.gev.ExternalProductSelect(op0, dset, sel, op0)
    assert np.array_equal(S.down(op0), ct)


@pytest.mark.parametrize("inplace", [False, True], ids=["out-of-place", "in-place"])
def test_select_pass_through_on_three_limb_polynomials(ctx, inplace):
    """keys of two limbs on polynomials of three: a pass-through entry copies limbs 0 and 1 and leaves limb 2 alone"""
    q, p = E.moduli(10, (35, 20, 45), (61,))
    S = Edge(ctx, 10, q, p, 7, E.ONE, level=1)
    rng = rng_for(10050)
    okey, dkey = S.rgsw(rng)
    dset = S.gev.NewKeySet([dkey])
    sel = [-1, 0, -1]
    ct = S.cts(rng, 3)
    want = np.stack([ct[b] if s < 0 else R.external_product(S.oev, ct[b], okey) for b, s in enumerate(sel)])
    got = _run_at_level(S, None, dset, ct, lambda a, k, o: S.gev.ExternalProductSelect(a, k, sel, o), inplace)
    assert np.array_equal(got, want)


# ---- H. the generic route's chunk loop -----------------------------------------------------------------------------------------------
def test_generic_route_chunks_a_batch_of_32768(ctx):
    """two chunks (32767 + 1 entries) at logN 8 -- below the one-launch kernel's rings -- with one 14-bit limb, one window and no
    special prime: about 0.7 GB of scratch per chunk; entries cycle over three ciphertexts and every entry is compared"""
    B, logN = 32768, 8
    S = Edge(ctx, logN, [E.Q14], [], 14, E.GEN)
    rng = rng_for(10100)
    orgsw, dkeys = S.rgsw(rng)
    assert orgsw[0].q.shape[0] == 1
    cts = S.cts(rng, 3)
    want3 = S.want(cts, orgsw)
    which = np.arange(B) % 3
    ct = cts[which]
    op0, out = S.up(ct), S.new_ct(B)
    S.gev.ExternalProduct(op0, dkeys, out)
    got = S.down(out)
    assert np.array_equal(got[-1], want3[which[-1]]), "the second chunk's entry"
    assert np.array_equal(got, want3[which])


# ---- I. the 32-bit branch's wrap bound -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pw2", range(1, 9))
@pytest.mark.parametrize("side", [0, 1], ids=["below", "above"])
def test_wrap_bound_sweep(ctx, side, pw2):
    """two primes on either side of 2^32 / sqrt(120): the device accepts exactly where 2 D (6q - 2)(q - 1) < 2^64 (pw2 = 3, ten
    windows, separates the two primes); an accepted call gives the oracle's words, a refused one writes nothing"""
    q = E.wrap_primes()[side]
    S = Edge(ctx, 10, [q], [], pw2, E.ONE)
    rng = rng_for(10200 + pw2)
    orgsw, dkeys = S.rgsw(rng)
    assert R.takes_32bit_branch(S.oQ, orgsw)
    holds = R.wrap_bound_holds(S.oQ, orgsw)
    assert holds == (pw2 >= 4 or (pw2 == 3 and side == 0))
    ct = S.cts(rng, 2)
    op0, out = S.up(ct), S.up(ct ^ np.uint64(1))
    if holds:
        S.gev.ExternalProduct(op0, dkeys, out)
        assert np.array_equal(S.down(out), S.want(ct, orgsw))
    else:
        with pytest.raises(la.HeringError) as e:
            S.gev._ev.ExternalProduct(op0, dkeys, out)
        assert e.value.code == EINVAL and "2^64" in str(e.value)
        assert np.array_equal(S.down(out), ct ^ np.uint64(1))
    assert np.array_equal(S.down(op0), ct)
