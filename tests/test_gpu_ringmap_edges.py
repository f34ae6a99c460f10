"""The ring-degree maps and the ring-packing kernels at their edges (`-m gpu`): ring_fold_kernel<2>, <4>, <0>, ring_replicate_kernel,
ring_stride_kernel<UP>, ring_split_kernel, ring_merge_kernel, expand_step_kernel, xpow2_fill_kernel, pack_pre_kernel and
pack_post_kernel through their entries (include/hering_ringswitch.h, include/hering_ringpack.h), against the reference's own sequence of
calls on the oracle, word for word, on the rings, operand families and shapes of tests/ringmap_edges.py (tests/test_ringmap_host.py
holds those sequences against the headers' closed forms in Python integers, and asserts what each planted family is built for).

Every polynomial is allocated with the ring's whole chain of limbs and carries sentinel words in the limbs above the level: a call at a
level below the top must leave them as uploaded, in every batch entry.  A guard polynomial allocated right after each output is
checked as well, and every input is checked unchanged.

Sections (NOTES.md, "The ring-degree maps and the ring-packing kernels at their edges"): A the ring-degree maps, B the ring maps of
Split and Merge, C the step kernels and the tables, D the ciphertext entries at the class boundaries, E the batch as gridDim.z."""
import ctypes as C
import gc

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd import _lib
from lattigo_amd import rlwe as R
from oracle import oracle as O
from tests import boundary as Bd
from tests import ringmap_edges as X
from tests import ringmap_ref as M
from tests import ringpack_ref as REF
from tests.gpu_common import ctx  # noqa: F401
from tests.helpers import rng_for
from tests.test_gpu_ringswitch import ref_apply

pytestmark = pytest.mark.gpu
U = np.uint64
SENTINEL = U(0xA5C3A5C35A3C5A3C)
B = X.BATCH


@pytest.fixture(autouse=True)
def _no_garbage_left_behind():
    """a la.Ring owns itself, so the rings a test drops are released by the cycle collector: collect them at the test's own boundaries
    (these tests make many rings)"""
    gc.collect()
    yield
    gc.collect()


class Rig:
    """one chain on the device, at every degree asked for (whole chain: a call at a lower level leaves the limbs above it alone)"""

    def __init__(self, ctx, mods, ci=False):
        self.ctx, self.mods, self.ci, self.nq, self._g = ctx, list(mods), ci, len(mods), {}

    def g(self, N):
        if N not in self._g:
            self._g[N] = la.Ring(self.ctx, N, self.mods, conjugate_invariant=self.ci)
        return self._g[N]

    def full(self, arr):
        """[B][level + 1][N] -> [B][chain][N], sentinel words in the limbs above"""
        arr = np.asarray(arr, dtype=U)
        full = np.full((arr.shape[0], self.nq, arr.shape[2]), SENTINEL, dtype=U)
        full[:, : arr.shape[1]] = arr
        return full

    def up(self, arr):
        """(polynomial, the words it holds)"""
        full = self.full(arr)
        return la.Poly(self.g(full.shape[2]), self.nq, full.shape[0]).upload(full), full

    def out(self, N, batch, init=None):
        """(output polynomial, guard polynomial allocated right after it), all sentinel words but `init`"""
        p, _ = self.up(init if init is not None else np.empty((batch, 0, N), dtype=U))
        return p, la.Poly(self.g(N), self.nq, 1).upload(np.full((1, self.nq, N), SENTINEL, dtype=U))


def _check(rig, out, level, want, what):
    """np.array_equal with the oracle's words; the first difference named as (form, ring, family, ..., modulus, entry, limb, position)"""
    p, guard = out
    got = p.download()
    want = np.asarray(want, dtype=U)
    if not np.array_equal(got[:, : level + 1], want):
        b, l, j = np.argwhere(got[:, : level + 1] != want)[0]
        raise AssertionError(f"{what}: modulus {rig.mods[l]:#x}, batch entry {b}, limb {l}, position {j}: device "
                             f"{int(got[b, l, j]):#x}, oracle {int(want[b, l, j]):#x} ({int((got[:, : level + 1] != want).sum())} words differ)")
    assert (got[:, level + 1:] == SENTINEL).all(), f"{what}: wrote above level {level}"
    if guard is not None:
        assert (guard.download() == SENTINEL).all(), f"{what}: wrote beside the batch"


def _unchanged(held, what):
    for p, full in held:
        assert np.array_equal(p.download(), full), f"{what}: an input changed"


def _rc(rc):
    _lib.check(rc)


# ---- A: the ring-degree maps --------------------------------------------------------------------------------------------------------
def _degree_maps(rig, n, gap, level, tag, fold_families=X.FOLD_FAMILIES, copy_families=X.COPY_FAMILIES, seed=9100):
    N, L, ci = n * gap, _lib.load(), rig.ci
    m = rig.mods[: level + 1]
    gl = rig.g(N)
    for fam in fold_families:
        for k, a in enumerate(X.fold_inputs(fam, m, n, gap, B, seed)):
            want = np.stack([M.ref_down_ntt(a[b], m, N, gap, ci) for b in range(B)])
            pin = rig.up(a)
            out = rig.out(n, B)
            _rc(L.he_switch_ring_degree_ntt(gl.h, level, pin[0].h, out[0].h))
            what = f"A fold {n} x {gap}, {tag}, family {fam}, page {k}"
            _check(rig, out, level, want, what)
            _unchanged([pin], what)
    for fam in copy_families:
        small, big = X.rows(fam, m, n, B, seed + 10), X.rows(fam, m, N, B, seed + 20)
        ps, pb = rig.up(small), rig.up(big)
        for entry, call in (("he_switch_ring_degree_ntt", lambda o: L.he_switch_ring_degree_ntt(0, level, ps[0].h, o.h)),
                            ("he_map_small_to_large_ntt", lambda o: L.he_map_small_to_large_ntt(ps[0].h, o.h, level))):
            out = rig.out(N, B)
            _rc(call(out[0]))
            _check(rig, out, level, M.ref_up_ntt(small.reshape(-1, n), gap).reshape(B, -1, N), f"A replicate ({entry}) {n} x {gap}, {tag}, family {fam}")
        out = rig.out(n, B)
        _rc(L.he_switch_ring_degree(level, pb[0].h, out[0].h))
        _check(rig, out, level, M.ref_stride_down(big, gap), f"A stride down {n} x {gap}, {tag}, family {fam}")
        pre = X.rows("uniform", m, N, B, seed + 30)  # the words between the multiples of gap keep their pre-call values
        out = rig.out(N, B, pre)
        _rc(L.he_switch_ring_degree(level, ps[0].h, out[0].h))
        _check(rig, out, level, M.ref_stride_up(small, gap, pre), f"A stride up {n} x {gap}, {tag}, family {fam}")
        _unchanged([ps, pb], f"A copies {n} x {gap}, {tag}, family {fam}")


@pytest.mark.parametrize("ci", [False, True])
@pytest.mark.parametrize("n,gap", X.DEGREE_SHAPES)
def test_a_ring_degree_maps(ctx, n, gap, ci):
    """the fold (gap 2 and 4: the templates; gap 8, 16, 256: the generic path at two, four and 64 loop trips), the replicate through
    both entries, stride down and stride up; batch 3; the top level, the one below and level 0; mixed chain, and 193 / 12289 where
    the large degree allows them"""
    for name, mods in X.rings_for(n * gap, ci).items():
        rig = Rig(ctx, mods, ci)
        for level in X.levels(rig.nq):
            _degree_maps(rig, n, gap, level, f"ci {ci}, ring {name}, level {level}")
    ctx.sync()


# ---- B: the ring maps of Split and Merge --------------------------------------------------------------------------------------------
def _split_merge(rig, N, level, tag, families=X.CANONICAL_FAMILIES, seed=9200):
    n = N // 2
    m = rig.mods[: level + 1]
    gN = rig.g(N)
    tw = X.merge_twiddles(N, rig.mods)
    for fam in families:
        for k, a in enumerate(X.split_inputs(fam, m, N, B, seed)):
            ref = [M.seq_split(a[b], m) for b in range(B)]
            for with_odd in (True, False):
                what = f"B split, odd half {with_odd}, N {N}, {tag}, family {fam}, page {k}"
                pin, ev, od = rig.up(a), rig.out(n, B), rig.out(n, B)
                R.SplitNTT(gN, level, pin[0], ev[0], od[0] if with_odd else None)
                _check(rig, ev, level, np.stack([r[0] for r in ref]), what + " (even)")
                if with_odd:
                    _check(rig, od, level, np.stack([r[1] for r in ref]), what + " (odd)")
                else:
                    _check(rig, od, -1, np.empty((B, 0, n), dtype=U), what + " (the absent operand's polynomial)")
                _unchanged([pin], what)
        for k, (e, o) in enumerate(X.pair_inputs("merge", fam, m, n, B, seed + 100, tw)):
            pe, po = rig.up(e), rig.up(o)
            for with_odd in (True, False):
                what = f"B merge, odd half {with_odd}, N {N}, {tag}, family {fam}, page {k}"
                out = rig.out(N, B)
                R.MergeNTT(gN, level, pe[0], po[0] if with_odd else None, out[0])
                _check(rig, out, level, np.stack([M.seq_merge(e[b], o[b] if with_odd else None, m) for b in range(B)]), what)
            _unchanged([pe, po], f"B merge, N {N}, {tag}, family {fam}, page {k}")


@pytest.mark.parametrize("N", X.PACK_DEGREES)
def test_b_split_and_merge_ring_maps(ctx, N):
    """he_ring_split_ntt and he_ring_merge_ntt, with and without the odd half (the absent operand's polynomial is not written)"""
    for name, mods in X.rings_for(N).items():
        rig = Rig(ctx, mods)
        for level in X.levels(rig.nq):
            _split_merge(rig, N, level, f"ring {name}, level {level}")
    ctx.sync()


# ---- C: the step kernels and the tables ---------------------------------------------------------------------------------------------
def _expand(rig, N, level, kk, tag, families=X.CANONICAL_FAMILIES, seed=9400):
    L, g, m = _lib.load(), rig.g(N), rig.mods[: level + 1]
    for fam in families:
        for pg, (a, t) in enumerate(X.pair_inputs("expand", fam, m, N, B, seed)):
            what = f"C expand step, N {N}, k {kk}, {tag}, family {fam}, page {pg}"
            cin, tmp = [a, np.ascontiguousarray(a[::-1])], [t, np.ascontiguousarray(t[::-1])]  # component 1: the entries in reverse
            ref = [[M.seq_expand(cin[c][b], tmp[c][b], m, kk) for b in range(B)] for c in range(2)]
            add = [np.stack([r[0] for r in ref[c]]) for c in range(2)]
            full = [np.concatenate([add[c], np.stack([r[1] for r in ref[c]])]) for c in range(2)]
            pin, ptmp = [rig.up(x) for x in cin], [rig.up(x) for x in tmp]
            out = [rig.out(N, 2 * B) for _ in range(2)]
            _rc(L.he_ringpack_expand_step(g.h, level, kk, 0, pin[0][0].h, pin[1][0].h, ptmp[0][0].h, ptmp[1][0].h, out[0][0].h, out[1][0].h))
            so = [rig.out(N, B) for _ in range(2)]
            _rc(L.he_ringpack_expand_step(g.h, level, kk, 1, pin[0][0].h, pin[1][0].h, ptmp[0][0].h, ptmp[1][0].h, so[0][0].h, so[1][0].h))
            ip = [rig.out(N, B, x) for x in cin]  # in place: the reference's Add(c0, tmp, c0)
            _rc(L.he_ringpack_expand_step(g.h, level, kk, 1, ip[0][0].h, ip[1][0].h, ptmp[0][0].h, ptmp[1][0].h, ip[0][0].h, ip[1][0].h))
            for c in range(2):
                _check(rig, out[c], level, full[c], what + f", component {c}")
                _check(rig, so[c], level, add[c], what + f", sum only, component {c}")
                _check(rig, ip[c], level, add[c], what + f", sum only in place, component {c}")
            _unchanged(pin + ptmp, what)


PAIRS = 6
KINDS = ("both", "a", "b")


def _pair_kind(z):
    """pair z takes its words from entry z mod 3 of a page (component 1: from the next entry); the kinds walk so that each entry is once a
    full pair and once a single operand"""
    return KINDS[(z + z // 3) % 3]


def _pack(rig, N, level, kk, tag, families=X.CANONICAL_FAMILIES, seed=9500):
    L, g, m = _lib.load(), rig.g(N), rig.mods[: level + 1]
    tw = X.pack_twiddles(N, rig.mods, kk)

    def run(form, fam, pg, x, y):
        """x / y: [B][limbs][N], the first and the second operand of the form (pre: a, b; post: the destination, T)"""
        what = f"C {form}, N {N}, k {kk}, {tag}, family {fam}, page {pg}"
        held = {"a": [], "b": []}  # per pair: None, or [((polynomial, words), wanted words) per component]
        Tin, Twant = np.empty((PAIRS, 2) + x.shape[1:], dtype=U), np.empty((PAIRS, 2) + x.shape[1:], dtype=U)
        for z in range(PAIRS):
            kind = _pair_kind(z)
            rows = {"a": [], "b": []}
            for c in range(2):
                xe, ye = x[(z + c) % B], y[(z + c) % B]
                if form == "pack_pre":
                    a, b = (xe if kind != "b" else None), (ye if kind != "a" else None)
                    a2, b2, Twant[z, c] = M.seq_pack_pre(a, b, m, kk)
                else:  # the destination is a where a is present, b otherwise; the b of a full pair is left alone
                    a, b = (xe if kind != "b" else None), (xe if kind == "b" else ye if kind == "both" else None)
                    Tin[z, c] = Twant[z, c] = ye
                    a2, b2 = M.seq_pack_post(a, b, ye, m)
                for name, before, after in (("a", a, a2), ("b", b, b2)):
                    if before is not None:
                        rows[name].append((rig.up(before[None]), after))
            for name in ("a", "b"):
                held[name].append(rows[name] or None)
        guard = la.Poly(g, rig.nq, 1).upload(np.full((1, rig.nq, N), SENTINEL, dtype=U))
        arrs = [R._harr([(pair[c][0][0] if pair else None) for pair in held[name]]) for name in ("a", "b") for c in range(2)]
        if form == "pack_pre":
            T = [rig.out(N, PAIRS) for _ in range(2)]
            _rc(L.he_ringpack_pack_pre(g.h, level, kk, PAIRS, *arrs, T[0][0].h, T[1][0].h))
        else:
            T = [(rig.up(Tin[:, c])[0], None) for c in range(2)]
            _rc(L.he_ringpack_pack_post(g.h, level, PAIRS, *arrs, T[0][0].h, T[1][0].h))
        for c in range(2):
            _check(rig, T[c], level, Twant[:, c], what + f", T, component {c}")  # (post leaves T)
        for z in range(PAIRS):
            for name in ("a", "b"):
                for c, (poly, after) in enumerate(held[name][z] or ()):
                    _check(rig, (poly[0], guard), level, after[None], what + f", pair {z} ({_pair_kind(z)}), {name}, component {c}")

    for fam in families:
        for pg, (a, b) in enumerate(X.pair_inputs("pack_pre", fam, m, N, B, seed + kk, tw)):
            run("pack_pre", fam, pg, a, b)
        for pg, (v, T) in enumerate(X.pair_inputs("pack_post", fam, m, N, B, seed + 100)):
            run("pack_post", fam, pg, v, T)


def _xpow2(rig, N, level, kk, tag):
    for div in (False, True):
        out = rig.out(N, B)
        R.XPow2NTT(rig.g(N), level, kk, div, out[0])
        want = M.seq_xpow2(N, rig.mods, kk, div, level + 1)
        _check(rig, out, level, np.stack([want] * B), f"C xpow2, N {N}, k {kk}, div {div}, {tag}")


@pytest.mark.parametrize("N", X.PACK_DEGREES)
def test_c_expand_step(ctx, N):
    """he_ringpack_expand_step full, sum_only and sum_only in place; k = 0, 1, logN - 2, logN - 1"""
    for name, mods in X.rings_for(N).items():
        rig = Rig(ctx, mods)
        for level in X.levels(rig.nq):
            for kk in X.table_indices(N.bit_length() - 1):
                _expand(rig, N, level, kk, f"ring {name}, level {level}")
    ctx.sync()


@pytest.mark.parametrize("N", X.PACK_DEGREES)
def test_c_pack_steps(ctx, N):
    """he_ringpack_pack_pre / _post over six pairs of all three kinds (a and b, a only, b only), each carrying the families"""
    assert sorted(_pair_kind(z) for z in range(PAIRS)) == sorted(KINDS * 2) and all(_pair_kind(e) != _pair_kind(e + B) for e in range(B))
    for name, mods in X.rings_for(N).items():
        rig = Rig(ctx, mods)
        for level in X.levels(rig.nq):
            for kk in X.table_indices(N.bit_length() - 1):
                _pack(rig, N, level, kk, f"ring {name}, level {level}")
    ctx.sync()


@pytest.mark.parametrize("N", X.PACK_DEGREES)
def test_c_monomial_tables(ctx, N):
    """he_ring_xpow2_ntt for both signs, every k, on a batch of three"""
    for name, mods in X.rings_for(N).items():
        rig = Rig(ctx, mods)
        for level in X.levels(rig.nq):
            for kk in range(N.bit_length() - 1):
                _xpow2(rig, N, level, kk, f"ring {name}, level {level}")
    ctx.sync()


# ---- the longest chain --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [X.RING_MAX_MODULI - 1, X.RING_MAX_MODULI - 2])
def test_a_c_most_limbs_in_one_launch(ctx, level):
    """48 limbs (gridDim.y = 48 at the top level, 47 below) at N = 32 -> 16 through one form of each kernel; the chain interleaves the
    three classes, so a limb that took a neighbour's constants gives other words.  A 49th modulus is refused."""
    with pytest.raises(la.HeringError):
        la.Ring(ctx, 32, X.chain49())
    rig = Rig(ctx, X.chain48())
    tag = f"48-limb chain, level {level}"
    fams = ("cred", "canonical", "uniform")
    _degree_maps(rig, 16, 2, level, tag, fold_families=fams, copy_families=("uniform",), seed=9700)
    _split_merge(rig, 32, level, tag, families=fams, seed=9710)
    _expand(rig, 32, level, 4, tag, families=fams, seed=9730)
    _pack(rig, 32, level, 4, tag, families=fams, seed=9740)
    _xpow2(rig, 32, level, 3, tag)
    ctx.sync()


# ---- D: the ciphertext entries at the class boundaries ------------------------------------------------------------------------------
def _key(words, rng, q, p, N):
    D = O.BaseRNSDecompositionVectorSize(len(q) - 1, len(p) - 1)
    kq = np.stack([np.stack([words(rng, q, N) for _ in range(2)]) for _ in range(D)])
    kp = np.stack([np.stack([words(rng, p, N) for _ in range(2)]) for _ in range(D)])
    return kq, kp


def _ct(words, rng, mods, N, batch):
    """[2][batch][limbs][N]"""
    return [np.stack([words(rng, mods, N) for _ in range(batch)]) for _ in range(2)]


def _d_chains(logN, ci=False):
    lr = logN + (1 if ci else 0)
    return Bd.class_chain(lr, "idhd"), Bd.class_chain(lr, "ih", skip={"i": 1, "h": 1})


def _d_check(got_polys, want, level, what):
    """want[b][k]: [level + 1][n]"""
    for k, p in enumerate(got_polys):
        got = p.download()
        for b in range(got.shape[0]):
            if not np.array_equal(got[b, : level + 1], want[b][k]):
                l, j = np.argwhere(got[b, : level + 1] != want[b][k])[0]
                raise AssertionError(f"{what}: component {k}, batch entry {b}, limb {l}, position {j}: device {int(got[b, l, j]):#x}, "
                                     f"oracle {int(want[b][k][l, j]):#x}")
            assert (got[b, level + 1:] == SENTINEL).all(), f"{what}: wrote above level {level}"


def _sentinel_ct(ring, nq, batch):
    return [la.Poly(ring, nq, batch).upload(np.full((batch, nq, ring.N), SENTINEL, dtype=U)) for _ in range(2)]


@pytest.mark.parametrize("logN,ci", [(12, False), (13, False), (12, True)])
def test_d_apply_evaluation_key_at_the_class_boundaries(ctx, logN, ci):
    """the down form of he_apply_evaluation_key at gap 2 and gap 4 and its up form; Q = class_chain("idhd"), P = class_chain("ih")
    further from the boundary; batch 2, the top level and the one below; ciphertext and key words from WordCycle(CANONICAL_KINDS)"""
    q, p = _d_chains(logN, ci)
    N, nq, batch = 1 << logN, len(q), 2
    rng = rng_for(9800 + logN + 100 * ci)
    words = Bd.WordCycle(Bd.CANONICAL_KINDS, logN)
    gQ, gP = la.Ring(ctx, N, q, conjugate_invariant=ci), la.Ring(ctx, N, p, conjugate_invariant=ci)
    oQ, oP = O.Ring(N, q, ci), O.Ring(N, p, ci)
    gev, oev = la.Evaluator(gQ, gP), O.Evaluator(oQ, oP)
    kq, kp = _key(words, rng, q, p, N)
    gk, ok = gev.NewEvaluationKey(kq, kp), O.EvaluationKey(kq, kp)
    small = {gap: la.Ring(ctx, N // gap, q, conjugate_invariant=ci) for gap in (2, 4)}
    for level in (nq - 1, nq - 2):
        m = q[: level + 1]
        big = _ct(words, rng, q, N, batch)
        pbig = [la.Poly(gQ, nq, batch).upload(x) for x in big]
        t = [ref_apply(oev, oQ, level, [big[0][b], big[1][b]], ok, ci) for b in range(batch)]
        for gap in (2, 4):
            out = _sentinel_ct(small[gap], nq, batch)
            gev.ApplyEvaluationKey(level, pbig, gk, out)
            want = [[M.ref_down_ntt(t[b][k], q, N, gap, ci) for k in range(2)] for b in range(batch)]
            _d_check(out, want, level, f"D apply evaluation key, down, gap {gap}, logN {logN}, ci {ci}, level {level}")
        assert all(np.array_equal(pbig[k].download(), big[k]) for k in range(2)), "inputs unchanged"
        gap = 2
        sm = _ct(words, rng, q, N // gap, batch)
        psm = [la.Poly(small[gap], nq, batch).upload(x) for x in sm]
        out = _sentinel_ct(gQ, nq, batch)
        gev.ApplyEvaluationKey(level, psm, gk, out)
        want = [ref_apply(oev, oQ, level, [M.ref_up_ntt(sm[k][b][: level + 1], gap) for k in range(2)], ok, ci) for b in range(batch)]
        _d_check(out, want, level, f"D apply evaluation key, up, gap {gap}, logN {logN}, ci {ci}, level {level}")
        assert all(np.array_equal(psm[k].download(), sm[k]) for k in range(2)), "inputs unchanged"
    ctx.sync()


@pytest.mark.parametrize("logN", [12, 13])
def test_d_ringpack_split_and_merge_at_the_class_boundaries(ctx, logN):
    """he_ringpack_split (with and without the odd halves) and he_ringpack_merge (with and without) on the same chains and words"""
    q, p = _d_chains(logN)
    N, n, nq, batch = 1 << logN, 1 << (logN - 1), len(q), 2
    rng = rng_for(9850 + logN)
    words = Bd.WordCycle(Bd.CANONICAL_KINDS, logN + 1)
    rings = {logN - 1: (O.Ring(n, q), O.Ring(n, p)), logN: (O.Ring(N, q), O.Ring(N, p))}
    keys = {(logN, logN - 1): _key(words, rng, q, p, N), (logN - 1, logN): _key(words, rng, q, p, N)}
    ref = REF.RingPackingEvaluator(rings, {ab: O.EvaluationKey(*k) for ab, k in keys.items()})
    gr = {d: (la.Ring(ctx, 1 << d, q), la.Ring(ctx, 1 << d, p)) for d in rings}
    gev = {d: la.Evaluator(*gr[d]) for d in gr}
    dev = R.RingPackingEvaluator(gev, {ab: gev[logN].NewEvaluationKey(*k) for ab, k in keys.items()})
    for level in (nq - 1, nq - 2):
        big = _ct(words, rng, q, N, batch)
        pbig = [la.Poly(gr[logN][0], nq, batch).upload(x) for x in big]
        want = [ref.Split(np.stack([big[0][b], big[1][b]])[:, : level + 1]) for b in range(batch)]
        even, odd = _sentinel_ct(gr[logN - 1][0], nq, batch), _sentinel_ct(gr[logN - 1][0], nq, batch)
        dev.Split(level, pbig, even, odd)
        _d_check(even, [w[0] for w in want], level, f"D split even, logN {logN}, level {level}")
        _d_check(odd, [w[1] for w in want], level, f"D split odd, logN {logN}, level {level}")
        even = _sentinel_ct(gr[logN - 1][0], nq, batch)
        dev.Split(level, pbig, even)
        _d_check(even, [w[0] for w in want], level, f"D split without the odd halves, logN {logN}, level {level}")
        assert all(np.array_equal(pbig[k].download(), big[k]) for k in range(2)), "inputs unchanged"
        he, ho = _ct(words, rng, q, n, batch), _ct(words, rng, q, n, batch)
        pe, po = ([la.Poly(gr[logN - 1][0], nq, batch).upload(x) for x in h] for h in (he, ho))
        cut = lambda h, b: np.stack([h[0][b], h[1][b]])[:, : level + 1]
        for with_odd in (True, False):
            out = _sentinel_ct(gr[logN][0], nq, batch)
            dev.Merge(level, pe, po if with_odd else None, out)
            _d_check(out, [ref.Merge(cut(he, b), cut(ho, b) if with_odd else None) for b in range(batch)], level,
                     f"D merge, odd halves {with_odd}, logN {logN}, level {level}")
        assert all(np.array_equal(pe[k].download(), he[k]) and np.array_equal(po[k].download(), ho[k]) for k in range(2)), "inputs unchanged"
    ctx.sync()


# ---- E: the batch as gridDim.z -----------------------------------------------------------------------------------------------------
E_BATCHES = (65535, 65536, 65537)
_e_cache = {}


def _e_reference():
    """one limb of modulus 193, n = 16, N = 32, for the largest batch (a smaller batch is its first entries): every word carries its
    entry number -- in full for the copies, which take any word, and modulo 193 for the fold, whose domain ends at 2q.  The fold's
    words are the oracle's INTT -> stride -> NTT, row by row through its C entries (65537 rows)."""
    if not _e_cache:
        Bm, n, N, q = max(E_BATCHES), 16, 32, X.Q193
        big, small, L = O.Ring(N, [q]), O.Ring(n, [q]), O.lib()
        e = np.arange(Bm, dtype=U)[:, None]
        xs = (U(1 << 40) + e * U(n) + np.arange(n, dtype=U)[None, :]).reshape(Bm, 1, n)
        xb = (U(1 << 41) + e * U(N) + np.arange(N, dtype=U)[None, :]).reshape(Bm, 1, N)
        xf = np.ascontiguousarray(((e + U(5) * np.arange(N, dtype=U)[None, :]) % U(q)).reshape(Bm, 1, N))
        pre = (~xb).copy()

        def rows(fn, h, src, width):
            dst = np.zeros_like(src)
            sa, da = src.ctypes.data, dst.ctypes.data
            for off in range(0, Bm * width * 8, width * 8):
                fn(h, 0, C.cast(sa + off, O.u64p), C.cast(da + off, O.u64p))
            return dst

        coeff = np.ascontiguousarray(rows(L.lo_intt, big._h, xf, N)[:, :, ::2])
        fold = rows(L.lo_ntt, small._h, coeff, n)
        for b in (0, 1, 192, 193, Bm - 1):  # the direct calls are the wrapper's
            assert np.array_equal(fold[b], M.ref_down_ntt(xf[b], [q], N, 2, False))
        _e_cache.update(xs=xs, xb=xb, xf=xf, pre=pre, fold=fold, replicate=np.repeat(xs, 2, axis=2), down=M.ref_stride_down(xb, 2),
                        up=M.ref_stride_up(xs, 2, pre))
    return _e_cache


@pytest.mark.parametrize("batch", E_BATCHES)
def test_e_batches_at_the_grid_limit(ctx, batch):
    """launch_ring_degree_fold_ntt, _replicate_ntt and _stride put the batch into gridDim.z, and rs_args checks no limit.  One
    193-modulus limb, n = 16, N = 32 (16 MB a polynomial).  The runtime takes gridDim.z = 65535, 65536 and 65537 alike for ew_kernel
    and its neighbours (NOTES.md), so the expected outcome is that every call is right in every entry -- include/hering_ringswitch.h
    states no limit for these entries and needs none -- and that the context serves a further call and syncs clean afterwards."""
    ref = _e_reference()
    L = _lib.load()
    g32, g16 = la.Ring(ctx, 32, [X.Q193]), la.Ring(ctx, 16, [X.Q193])
    ps, pb, pf = (la.Poly(g, 1, batch).upload(ref[k][:batch]) for g, k in ((g16, "xs"), (g32, "xb"), (g32, "xf")))
    sent = lambda N: np.full((batch, 1, N), SENTINEL, dtype=U)
    calls = {"fold": (g16, sent(16), lambda o: L.he_switch_ring_degree_ntt(g32.h, 0, pf.h, o.h)),
             "replicate": (g32, sent(32), lambda o: L.he_map_small_to_large_ntt(ps.h, o.h, 0)),
             "down": (g16, sent(16), lambda o: L.he_switch_ring_degree(0, pb.h, o.h)),
             "up": (g32, ref["pre"][:batch], lambda o: L.he_switch_ring_degree(0, ps.h, o.h))}
    s1 = la.Poly(g16, 1, 1).upload(ref["xs"][:1])
    for name, (g, init, call) in calls.items():
        out = la.Poly(g, 1, batch).upload(init)
        _rc(call(out))
        got, want = out.download(), ref[name][:batch]
        if not np.array_equal(got, want):
            b, l, j = np.argwhere(got != want)[0]
            raise AssertionError(f"E {name}, modulus 0xc1, family entry-number, batch {batch}: entry {b}, limb {l}, position {j}: device {int(got[b, l, j]):#x}, "
                                 f"oracle {int(want[b, l, j]):#x} ({int((got != want).any(axis=(1, 2)).sum())} entries differ)")
        o1 = la.Poly(g32, 1, 1)
        _rc(L.he_map_small_to_large_ntt(s1.h, o1.h, 0))  # the context serves the next call
        assert np.array_equal(o1.download(), ref["replicate"][:1]), name
        ctx.sync()
    for p, k in ((ps, "xs"), (pb, "xb"), (pf, "xf")):
        assert np.array_equal(p.download(), ref[k][:batch]), f"E input {k} changed"
