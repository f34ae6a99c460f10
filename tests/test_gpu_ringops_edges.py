"""The coefficient-wise ring operations at their word and shape edges (`-m gpu`): everything of ring/operations.go on the device --
the 33 instantiations of ew_kernel, the double-scalar form, shift_kernel (Shift, MultByMonomial), gather_kernel<ADD> and the two
coefficient automorphisms -- against the oracle, word for word, on the rings, operand families, scalars, shifts and Galois
elements of tests/ringops_edges.py (tests/test_ringops_host.py holds the oracle against ring/vec_ops.go in Python integers).

Every output polynomial is allocated with the ring's whole chain of limbs and filled with sentinel words first: a call at a
level below the top must leave the limbs above it as uploaded, in every batch entry (entry b's limbs above the level lie
between its written limbs and entry b + 1's).  The interface has no call on part of a batch, so the words beside the LAST entry
written are those of a guard polynomial allocated right after the output, checked as well.

Sections (NOTES.md, "The coefficient-wise ring operations at their edges"): A words, B moduli, C geometry, D scalars,
E permutations, F the batch as gridDim.z, G concurrent callers that differ only in a parameter."""
import threading

import numpy as np
import pytest

import lattigo_amd as la
from oracle import oracle as O
from tests import ringops_edges as E
from tests.gpu_common import ctx  # noqa: F401
from tests.helpers import rng_for

pytestmark = pytest.mark.gpu
U = np.uint64
M64 = E.M64
SENTINEL = U(0xA5C3A5C35A3C5A3C)
BIN = list(la.ring.BINOPS)
UN = list(la.ring.UNOPS)
SC = list(la.ring.SCALAROPS)
BIGINT = ("AddScalarBigint", "SubScalarBigint", "MulScalarBigint", "MulScalarBigintThenAdd")
DOUBLE = ("AddDoubleRNSScalar", "SubDoubleRNSScalar", "MulDoubleRNSScalar", "MulDoubleRNSScalarThenAdd")


class Rig:
    """one ring on the device (whole chain) and in the oracle (one ring per level)"""

    def __init__(self, ctx, N, mods, ci=False):
        self.N, self.mods, self.ci, self.nq = N, list(mods), ci, len(mods)
        self.g = la.Ring(ctx, N, self.mods, conjugate_invariant=ci)
        self._o = {}

    def o(self, level):
        if level not in self._o:
            self._o[level] = O.Ring(self.N, self.mods[: level + 1], self.ci)
        return self._o[level]

    def up(self, arr, B):
        """[B][level + 1][N] -> a polynomial of the whole chain, sentinel words in the limbs above"""
        arr = np.asarray(arr, dtype=U)
        full = np.full((B, self.nq, self.N), SENTINEL, dtype=U)
        full[:, : arr.shape[1]] = arr
        return la.Poly(self.g, self.nq, B).upload(full)

    def out(self, B, init=None):
        """(output polynomial, guard polynomial allocated right after it), all sentinel words but `init`"""
        p = self.up(init if init is not None else np.empty((B, 0, self.N), dtype=U), B)
        return p, la.Poly(self.g, self.nq, 1).upload(np.full((1, self.nq, self.N), SENTINEL, dtype=U))


def _check(rig, out, level, want, what):
    """np.array_equal with the oracle's words; the first difference named as (form, modulus, family, ..., entry, limb, position)"""
    p, guard = out
    got = p.download()
    want = np.asarray(want, dtype=U)
    if not np.array_equal(got[:, : level + 1], want):
        b, l, j = np.argwhere(got[:, : level + 1] != want)[0]
        raise AssertionError(f"{what}: modulus {rig.mods[l]:#x}, batch entry {b}, limb {l}, position {j}: device "
                             f"{int(got[b, l, j]):#x}, oracle {int(want[b, l, j]):#x} ({int((got[:, : level + 1] != want).sum())} words differ)")
    assert (got[:, level + 1:] == SENTINEL).all(), f"{what}: wrote above level {level}"
    assert (guard.download() == SENTINEL).all(), f"{what}: wrote beside the batch"


def _per_entry(fn, B, *ops):
    """the oracle entry by entry; an operand of batch 1 serves every entry"""
    return np.stack([fn(*[(a[b] if a.shape[0] > 1 else a[0]) for a in ops]) for b in range(B)])


def _binary(rig, level, name, x, y, z, B, what):
    """x, y: [B or 1][level + 1][N] (batch 1: broadcast over the batch); z: [B][..][N], the destination's words before the call"""
    o = rig.o(level)
    want = _per_entry(lambda a, b, c: o.binop(name, a, b, c), B, x, y, z)
    out = rig.out(B, z)
    getattr(rig.g.AtLevel(level), name)(rig.up(x, x.shape[0]), rig.up(y, y.shape[0]), out[0])
    _check(rig, out, level, want, what)


def _unary(rig, level, name, x, B, what):
    want = _per_entry(lambda a: rig.o(level).unop(name, a), B, x)
    out = rig.out(B)
    getattr(rig.g.AtLevel(level), name)(rig.up(x, B), out[0])
    _check(rig, out, level, want, what)


def _scalar(rig, level, name, x, s, z, B, what):
    want = _per_entry(lambda a, c: rig.o(level).scalarop(name, a, s, c), B, x, z)
    out = rig.out(B, z)
    getattr(rig.g.AtLevel(level), name)(rig.up(x, B), s, out[0])
    _check(rig, out, level, want, what)


def _bigint(rig, level, name, x, s, z, B, what):
    o = rig.o(level)
    want = _per_entry((lambda a, c: o.MulScalarBigintThenAdd(a, s, c)) if name.endswith("ThenAdd") else (lambda a, c: getattr(o, name)(a, s)), B, x, z)
    out = rig.out(B, z)
    getattr(rig.g.AtLevel(level), name)(rig.up(x, B), s, out[0])  # (a negative scalar goes through the wrapper's _nonneg)
    _check(rig, out, level, want, what)


def _double(rig, level, name, x, s0, s1, z, B, what):
    o = rig.o(level)
    s0, s1 = s0[: level + 1], s1[: level + 1]
    want = _per_entry((lambda a, c: getattr(o, name)(a, s0, s1, c)) if name.endswith("ThenAdd") else (lambda a, c: getattr(o, name)(a, s0, s1)), B, x, z)
    out = rig.out(B, z)
    getattr(rig.g.AtLevel(level), name)(rig.up(x, B), s0, s1, out[0])
    _check(rig, out, level, want, what)


def _rns(rig, level, x, sc, B, what):
    want = _per_entry(lambda a: rig.o(level).MulRNSScalarMontgomery(a, sc[: level + 1]), B, x)
    out = rig.out(B)
    rig.g.AtLevel(level).MulRNSScalarMontgomery(rig.up(x, B), sc[: level + 1], out[0])
    _check(rig, out, level, want, what)


def _vector(rig, level, x, vec, z, B, what):
    o = rig.o(level)
    pv = la.Poly(rig.g, 1).upload(vec[None, None, :])
    for add in (False, True):
        want = _per_entry((lambda a, c: o.MulByVectorMontgomery(a, vec, c)) if add else (lambda a, c: o.MulByVectorMontgomery(a, vec)), B, x, z)
        out = rig.out(B, z)
        getattr(rig.g.AtLevel(level), "MulByVectorMontgomeryThenAddLazy" if add else "MulByVectorMontgomery")(rig.up(x, B), pv, out[0])
        _check(rig, out, level, want, f"{what}, then add lazy: {add}")


def _pages(fam, rig, level, B, seed, form=None, scalar=None, n_uniform=E.N_UNIFORM):
    cols = E.poly_cols(fam, rig.mods[: level + 1], seed, form, scalar, n_uniform)
    return [] if cols is None else E.lay(cols, rig.N, B)


def _a_scalars(mods):
    return (mods[0] - 1, 2 * mods[0], M64)


def _all_forms(rig, level, B, families, seed, tag, broadcast=False, vectors=False, n_uniform=E.N_UNIFORM):
    """every binary, unary and scalar form (three scalars) on the families; broadcast: each binary form also with its first, its
    second and both operands a batch-1 polynomial"""
    mods = rig.mods[: level + 1]
    for fam in families:
        for name in BIN:
            for k, (x, y, z) in enumerate(_pages(fam, rig, level, B, seed, form=name, n_uniform=n_uniform)):
                for bc in ((0, 1, 2, 3) if broadcast else (0,)):
                    _binary(rig, level, name, x[:1] if bc & 1 else x, y[:1] if bc & 2 else y, z, B, f"{tag} {name}, family {fam}, page {k}, broadcast {bc}")
        for k, (x, y, z) in enumerate(_pages(fam, rig, level, B, seed + 100, n_uniform=n_uniform)):
            for name in UN:
                _unary(rig, level, name, x, B, f"{tag} {name}, family {fam}, page {k}")
            if vectors:
                for sc in E.rns_scalars(mods):
                    _rns(rig, level, x, sc, B, f"{tag} MulRNSScalarMontgomery, family {fam}, page {k}")
                vec = np.ascontiguousarray(_pages("word64", rig, level, 1, seed + 300)[0][1][0, 0])  # a vector of 64-bit edges
                _vector(rig, level, x, vec, z, B, f"{tag} MulByVectorMontgomery, family {fam}, page {k}")
        for name in SC:
            for s in _a_scalars(mods):
                for k, (x, y, z) in enumerate(_pages(fam, rig, level, B, seed + 200, form=name, scalar=s, n_uniform=n_uniform)):
                    _scalar(rig, level, name, x, s, z, B, f"{tag} {name}({s:#x}), family {fam}, page {k}")


# ---- A: words ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", E.FAMILIES)
def test_a_every_form_on_every_word_family(ctx, family):
    """mixed chain, N = 1024 (two workgroups of ew_kernel, four of the others), top level, batch 3"""
    rig = Rig(ctx, 1024, E.mixed_chain(10))
    _all_forms(rig, rig.nq - 1, 3, [family], 6100, "A", broadcast=True, vectors=True)


# ---- B: moduli --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("chain", ["q97", "q12289", "mixed+27", "q12289@512"])
def test_b_edge_families_at_the_extreme_moduli(ctx, chain, B):
    """97 (the extreme Barrett constants), 12289, and the mixed chain with a 27-bit prime after it, N = 16 (12289 at N = 512 too)"""
    N = 512 if chain.endswith("@512") else 16
    mods = {"q97": (E.Q97,), "q12289": (E.Q12289,), "q12289@512": (E.Q12289,), "mixed+27": E.mixed_chain(4, True)}[chain]
    rig = Rig(ctx, N, mods)
    _all_forms(rig, rig.nq - 1, B, E.EDGE_FAMILIES, 6200, f"B {chain}")


# ---- C: geometry ------------------------------------------------------------------------------------------------------------------
def _permutations(rig, level, B, x, tag, shifts, gals, acc=None, inplace=True):
    """Shift and MultByMonomial (out of place and in place), Automorphism, and on a standard ring the gather with and without the
    add; x: [B][level + 1][N]"""
    g, o = rig.g.AtLevel(level), rig.o(level)
    for k in shifts:
        for name, fn in (("Shift", o.Shift), ("MultByMonomial", o.MultByMonomial)):
            want = _per_entry(lambda a: fn(a, k), B, x)
            out = rig.out(B)
            getattr(g, name)(rig.up(x, B), k, out[0])
            _check(rig, out, level, want, f"{tag} {name}({k}), family permutation")
            if inplace:
                out = rig.out(B, x)
                getattr(g, name)(out[0], k, out[0])
                _check(rig, out, level, want, f"{tag} {name}({k}) in place, family permutation")
    for gal in gals:
        want = _per_entry(lambda a: o.Automorphism(a, gal), B, x)
        out = rig.out(B)
        g.Automorphism(rig.up(x, B), gal, out[0])
        _check(rig, out, level, want, f"{tag} Automorphism({gal:#x}), ci {rig.ci}, family permutation")
        if rig.ci:
            continue  # (the NTT index table of a conjugate-invariant ring stays below N only for elements = 1 mod 4)
        idx = g.AutomorphismNTTIndex(gal)
        table = idx.download()
        assert np.array_equal(table, o.AutomorphismNTTIndex(gal)) and table.max() < rig.N, f"{tag} AutomorphismNTTIndex({gal:#x})"
        want = _per_entry(lambda a: o.AutomorphismNTTWithIndex(a, table), B, x)
        out = rig.out(B)
        g.AutomorphismNTTWithIndex(rig.up(x, B), idx, out[0])
        _check(rig, out, level, want, f"{tag} AutomorphismNTTWithIndex({gal:#x}), family permutation")
        want = _per_entry(lambda a, c: o.AutomorphismNTTWithIndexThenAddLazy(a, table, c), B, x, acc)
        out = rig.out(B, acc)
        g.AutomorphismNTTWithIndexThenAddLazy(rig.up(x, B), idx, out[0])
        _check(rig, out, level, want, f"{tag} AutomorphismNTTWithIndexThenAddLazy({gal:#x}), family wrap")


def _perm_operands(rig, level, B, seed):
    """x: zeros under every sign case, lazy and 64-bit words (entry b rotated by 3 b); acc: 64-bit words, half of them within 2q
    of 2^64 so that the lazy add wraps and does not"""
    mods = rig.mods[: level + 1]
    x0 = E.permutation_operand(mods, rig.N, seed)
    x = np.stack([np.roll(x0, 3 * b, axis=1) for b in range(B)])
    rng = rng_for(seed + 1)
    acc = E.Bd.wild_words(rng, x.shape)
    acc[:, :, ::2] = U(M64) - rng.integers(0, 2 * min(mods), size=acc[:, :, ::2].shape, dtype=U)
    return x, acc


@pytest.mark.parametrize("N", [16, 256, 512, 1024])
def test_c_degrees_and_levels(ctx, N):
    """one ew form with a product and one without, Shift, MultByMonomial, the gather with and without the add, and the coefficient
    automorphism on both ring types, at the top level, the one below and level 0 (batch 2): N = 16 is less than a wave, 256 one
    workgroup of the one-word kernels and half a workgroup of ew_kernel, 512 two and one, 1024 four and two"""
    logN = N.bit_length() - 1
    for ci in (False, True):
        rig = Rig(ctx, N, E.mixed_chain(logN, ci=ci), ci=ci)
        for level in (rig.nq - 1, rig.nq - 2, 0):
            tag = f"C N={N} level {level}"
            for fam in ("uniform", "lazy"):
                for name in ("MulCoeffsMontgomeryThenAdd", "Sub"):
                    for k, (x, y, z) in enumerate(_pages(fam, rig, level, 2, 6300, form=name, n_uniform=2 * N)):
                        _binary(rig, level, name, x, y, z, 2, f"{tag} {name}, family {fam}, page {k}")
            x, acc = _perm_operands(rig, level, 2, 6310)
            _permutations(rig, level, 2, x, tag, (1, N - 1, N + 1), (5, 2 * N - 1), acc)


RING_MAX_MODULI = 48  # he_ring_create refuses more


@pytest.mark.parametrize("level", [RING_MAX_MODULI - 1, RING_MAX_MODULI - 2])
def test_c_most_limbs_in_one_launch(ctx, level):
    """the launches take up to kMaxLimbs = 64 limbs (uint8_t limb tables, gridDim.y), but he_ring_create takes at most 48 moduli, so
    48 is the most limbs one of these entries can be asked for: gridDim.y = 48 at the top level, 47 below.  Every limb's result is
    under its own modulus (the chain interleaves the three classes, so a limb that took a neighbour's constants gives other
    words).  The 64 primes of the chain are refused as a ring."""
    with pytest.raises(la.HeringError):
        la.Ring(ctx, 16, E.chain64())
    rig = Rig(ctx, 16, E.chain64()[:RING_MAX_MODULI])
    tag = f"C 48 limbs level {level}"
    for fam in ("canonical", "lazy", "uniform"):
        for k, (x, y, z) in enumerate(_pages(fam, rig, level, 2, 6400, n_uniform=64)):
            for name in ("Add", "MulCoeffsMontgomery"):
                _binary(rig, level, name, x, y, z, 2, f"{tag} {name}, family {fam}, page {k}")
            _scalar(rig, level, "MulScalar", x, rig.mods[0] + 1, z, 2, f"{tag} MulScalar, family {fam}, page {k}")
    x, acc = _perm_operands(rig, level, 2, 6410)
    _permutations(rig, level, 2, x, tag, (3, 16 + 5), (5, 31), acc)
    # canonical words in, canonical words out, limb by limb
    xs = np.stack([np.stack([np.full(16, q - 1, dtype=U) for q in rig.mods[: level + 1]])])
    out = rig.out(1)
    rig.g.AtLevel(level).Add(rig.up(xs, 1), rig.up(xs, 1), out[0])
    got = out[0].download()[0, : level + 1]
    assert np.array_equal(got[:, 0], np.array([q - 2 for q in rig.mods[: level + 1]], dtype=U))


@pytest.mark.parametrize("N", [16, 1024, 2048])
def test_c_double_scalar_boundary(ctx, N):
    """the scalar switches at j >= N/2: inside a wave (N = 16), on a workgroup boundary of ew_kernel (1024: 512 words a workgroup),
    in mid-grid (2048); s0 != s1 in every limb, so a word on the wrong side of N/2 differs"""
    rig = Rig(ctx, N, E.mixed_chain(N.bit_length() - 1))
    pairs = E.double_scalars(rig.mods)
    for level in (rig.nq - 1, 0):
        for fam in ("canonical", "word64", "uniform"):
            for k, (x, y, z) in enumerate(_pages(fam, rig, level, 2, 6500, n_uniform=2 * N)[:2]):
                for s0, s1 in (pairs if N == 16 else pairs[2:5]):
                    for name in DOUBLE:
                        _double(rig, level, name, x, s0, s1, z, 2, f"C N={N} level {level} {name}, family {fam}, page {k}")


@pytest.mark.parametrize("N", [16, 512])
def test_c_conjugate_invariant_ring(ctx, N):
    rig = Rig(ctx, N, E.mixed_chain(N.bit_length() - 1, ci=True), ci=True)
    _all_forms(rig, rig.nq - 1, 2, E.EDGE_FAMILIES, 6600, f"C ci N={N}")


# ---- D: scalars -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top", [True, False])
def test_d_every_scalar_through_every_scalar_form(ctx, top):
    """0, 1, q0 - 1, q0, q0 + 1, q_last, 2 q0, 2^63, 2^64 - 1 through the five scalar forms; the product of the chain and +- 1, -1,
    a negative multiple of q0 and a 301-bit number through the bigint forms; 0 / q_i - 1 / q_i / 2^64 - 1 per limb through
    MulRNSScalarMontgomery; pairs of them through the double-scalar forms"""
    rig = Rig(ctx, 16, E.mixed_chain(4))
    level = rig.nq - 1 if top else 0
    mods = rig.mods[: level + 1]
    tag = f"D level {level}"
    for fam in E.EDGE_FAMILIES + ("cred",):
        for name in SC:
            for s in E.scalars(mods):
                for k, (x, y, z) in enumerate(_pages(fam, rig, level, 2, 6700, form=name, scalar=s)):
                    _scalar(rig, level, name, x, s, z, 2, f"{tag} {name}({s:#x}), family {fam}, page {k}")
    for fam in E.EDGE_FAMILIES:
        for k, (x, y, z) in enumerate(_pages(fam, rig, level, 2, 6710)):
            for s in E.bigint_scalars(mods):
                for name in BIGINT:
                    _bigint(rig, level, name, x, s, z, 2, f"{tag} {name}({s:#x}), family {fam}, page {k}")
            for sc in E.rns_scalars(rig.mods):
                _rns(rig, level, x, sc, 2, f"{tag} MulRNSScalarMontgomery, family {fam}, page {k}")
            if k == 0:
                for s0, s1 in E.double_scalars(rig.mods):
                    for name in DOUBLE:
                        _double(rig, level, name, x, s0, s1, z, 2, f"{tag} {name}, family {fam}")


# ---- E: permutations --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [False, True])
@pytest.mark.parametrize("N", [16, 512])
def test_e_every_shift_and_galois_element(ctx, N, ci):
    """k in {0, 1, N - 1, N, N + 1, 2N - 1, 2N, 2N + 7, -1, -N - 2, 2^31 - 1, -2^31} through Shift and MultByMonomial, out of place
    and in place; the Galois elements 1, 3, 5, N + 1, 2N - 1, 5^77 and the unreduced 2N + 5, 2^63 + 5, 2^64 - 1 through
    Automorphism (both ring types) and AutomorphismNTTIndex + WithIndex + WithIndexThenAddLazy (accumulator from the wrapping
    family); batch 2"""
    logN = N.bit_length() - 1
    rig = Rig(ctx, N, E.mixed_chain(logN, N == 16, ci=ci), ci=ci)
    level = rig.nq - 1
    x, acc = _perm_operands(rig, level, 2, 6800)
    _permutations(rig, level, 2, x, f"E N={N}", () if ci else E.shifts(N), E.galois_elements(N), acc)


# ---- F: the batch as gridDim.z ----------------------------------------------------------------------------------------------------
F_BATCHES = (65535, 65536, 65537)
_f_cache = {}


def _f_reference():
    """operands whose words carry their entry number (16 b + j, far above q = 97) and the oracle's words for the five calls, once,
    for the largest batch; a smaller batch is its first entries.  (The oracle's C entries directly, row by row: 65537 rows.)"""
    if not _f_cache:
        import ctypes as C
        B, N = max(F_BATCHES), 16
        o, L = O.Ring(N, [E.Q97]), O.lib()
        x = (np.arange(B * N, dtype=U)).reshape(B, 1, N)
        y = x * U(3) + U(1)
        table = o.AutomorphismNTTIndex(5)
        tp = table.ctypes.data_as(O.u64p)

        def rows(fn):
            out = np.zeros_like(x)
            xa, ya, oa = x.ctypes.data, y.ctypes.data, out.ctypes.data
            for off in range(0, B * N * 8, N * 8):
                fn(C.cast(xa + off, O.u64p), C.cast(ya + off, O.u64p), C.cast(oa + off, O.u64p))
            return out

        h = o._h
        _f_cache.update(x=x, y=y, table=table,
                        Add=rows(lambda a, b, c: L.lo_binop(h, 0, O.BINOPS["Add"], a, b, c)),
                        AddScalar=rows(lambda a, b, c: L.lo_scalarop(h, 0, O.SCALAROPS["AddScalar"], a, 1 << 63, c)),
                        Shift=o.Shift(x.reshape(B, N), 5).reshape(B, 1, N),  # (a permutation of positions: the rows as limbs)
                        Gather=rows(lambda a, b, c: L.lo_automorphism_ntt_with_index(h, 0, a, tp, c)),
                        Automorphism=rows(lambda a, b, c: L.lo_automorphism(h, 0, a, 3, c)))
        for b in (0, 1, B - 1):  # the direct calls are the wrapper's
            assert np.array_equal(_f_cache["Add"][b], o.binop("Add", x[b], y[b])) and np.array_equal(_f_cache["Automorphism"][b], o.Automorphism(x[b], 3))
    return _f_cache


@pytest.mark.parametrize("B", F_BATCHES)
def test_f_batches_at_the_grid_limit(ctx, B):
    """launch_ew_impl, launch_shift_impl, launch_gather and launch_automorphism_coeff put the batch into gridDim.z.  One
    97-modulus limb at N = 16 (8 MB a polynomial).  Measured on the MI355X (NOTES.md): the runtime takes gridDim.z = 65535, 65536
    and 65537 alike, so every call is right in every entry -- include/hering.h states no limit for these entries and needs
    none -- and the context serves a further call and syncs clean afterwards."""
    ref = _f_reference()
    g = la.Ring(ctx, 16, [E.Q97])
    x, y = ref["x"][:B], ref["y"][:B]
    px, py = la.Poly(g, 1, B).upload(x), la.Poly(g, 1, B).upload(y)
    idx = g.AutomorphismNTTIndex(5)
    assert np.array_equal(idx.download(), ref["table"])
    calls = {"Add": lambda out: g.Add(px, py, out), "AddScalar": lambda out: g.AddScalar(px, 1 << 63, out), "Shift": lambda out: g.Shift(px, 5, out),
             "Gather": lambda out: g.AutomorphismNTTWithIndex(px, idx, out), "Automorphism": lambda out: g.Automorphism(px, 3, out)}
    sent = np.full((B, 1, 16), SENTINEL, dtype=U)
    for name, call in calls.items():
        out = la.Poly(g, 1, B).upload(sent)
        call(out)
        got = out.download()
        if not np.array_equal(got, ref[name][:B]):
            b, l, j = np.argwhere(got != ref[name][:B])[0]
            raise AssertionError(f"F {name}, modulus 0x61, family entry-number, batch {B}: entry {b}, limb {l}, position {j}: device {int(got[b, l, j]):#x}, "
                                 f"oracle {int(ref[name][b, l, j]):#x}")
        small = la.Poly(g, 1, 1)
        g.Add(la.Poly(g, 1, 1).upload(x[:1]), la.Poly(g, 1, 1).upload(y[:1]), small)  # the context serves the next call
        assert np.array_equal(small.download(), ref["Add"][:1]), name
        ctx.sync()


# ---- G: concurrent callers that differ only in a parameter ------------------------------------------------------------------------
def _run_threads(fns):
    gate, errs = threading.Barrier(len(fns)), []

    def wrap(f):
        try:
            gate.wait()
            f()
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=wrap, args=(f,)) for f in fns]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs


def _g_cases(rig, rigs2):
    """name -> (K, make(k) -> (call(out), want, level, init)): caller k's call on polynomials of its own and the oracle's words
    for ITS parameter.  The queue merges requests whose key (op, par[], blob) matches: scalars live in the blob, the shift, the
    Galois element and the level in par."""
    N, mods, top = rig.N, rig.mods, rig.nq - 1
    rng = rng_for(6900)
    o = rig.o(top)
    xs = [np.stack([E.permutation_operand(mods, N, 6900 + k)]) for k in range(8)]
    for k in range(8):
        xs[k][0, :, 1::2] = np.stack([rng.integers(0, q, size=N // 2, dtype=U) for q in mods])
    ys = [np.stack([np.stack([rng.integers(0, q, size=N, dtype=U) for q in mods])]) for k in range(8)]
    px = [rig.up(x, 1) for x in xs]
    py = [rig.up(y, 1) for y in ys]
    g = rig.g
    sc = E.scalars(mods)[1:]  # eight scalars: 1, q0 - 1, q0, q0 + 1, q_last, 2 q0, 2^63, 2^64 - 1
    big = E.bigint_scalars(mods) + [7, (1 << 64) + 3]
    dbl = E.double_scalars(mods)
    ks = [1, 7, N - 1, N, N + 1, N + 9, 2 * N - 1, -3]
    gals = E.galois_elements(N)[1:]
    idx = [g.AutomorphismNTTIndex(gals[k // 2]) for k in range(8)]  # four elements, two callers each on tables of their own
    tables = [i.download() for i in idx]
    lo = top - 2
    olo = rig.o(lo)
    return {
        "AddScalar": lambda k: (lambda out: g.AddScalar(px[k], sc[k], out), o.scalarop("AddScalar", xs[k][0], sc[k]), top, None),
        "MulScalarThenSub": lambda k: (lambda out: g.MulScalarThenSub(px[k], sc[k], out), o.scalarop("MulScalarThenSub", xs[k][0], sc[k], ys[k][0]), top, ys[k]),
        "MulDoubleRNSScalar": lambda k: (lambda out: g.MulDoubleRNSScalar(px[k], dbl[k][0], dbl[k][1], out), o.MulDoubleRNSScalar(xs[k][0], *dbl[k]), top, None),
        "MulScalarBigint": lambda k: (lambda out: g.MulScalarBigint(px[k], big[k], out), o.MulScalarBigint(xs[k][0], big[k]), top, None),
        "Shift": lambda k: (lambda out: g.Shift(px[k], ks[k], out), o.Shift(xs[k][0], ks[k]), top, None),
        "MultByMonomial": lambda k: (lambda out: g.MultByMonomial(px[k], ks[k], out), o.MultByMonomial(xs[k][0], ks[k]), top, None),
        "Automorphism": lambda k: (lambda out: g.Automorphism(px[k], gals[k], out), o.Automorphism(xs[k][0], gals[k]), top, None),
        "AutomorphismNTTWithIndex": lambda k: (lambda out: g.AutomorphismNTTWithIndex(px[k], idx[k], out), o.AutomorphismNTTWithIndex(xs[k][0], tables[k]), top, None),
        "Add at two levels": lambda k: ((lambda out: g.AtLevel(lo).Add(px[k], py[k], out), olo.binop("Add", xs[k][0, : lo + 1], ys[k][0, : lo + 1]), lo, None) if k & 1 else
                                        (lambda out: g.Add(px[k], py[k], out), o.binop("Add", xs[k][0], ys[k][0]), top, None)),
        # half the callers pass the SAME batch-1 polynomial as second operand into an output of batch 2
        "Add with a broadcast operand": lambda k: ((lambda out: g.Add(rigs2[k], py[0], out), np.stack([o.binop("Add", np.roll(xs[k][0], b, axis=1), ys[0][0]) for b in range(2)]), top, None)
                                                   if k & 1 else (lambda out: g.Add(px[k], py[k], out), o.binop("Add", xs[k][0], ys[k][0]), top, None)),
    }, xs


@pytest.mark.parametrize("deferred", [0, 4])
def test_g_callers_that_differ_only_in_a_parameter(ctx, deferred):
    """SetCoalescing on (and once more with SetDeferred(4)): eight threads at once, each on polynomials of its own with a scalar,
    shift, Galois element, index table, level or broadcast shape of its own; every caller gets the oracle's words for ITS
    parameter.  N = 512, mixed chain."""
    rig = Rig(ctx, 512, E.mixed_chain(9))
    xs2 = None
    try:
        ctx.SetCoalescing(0, 0)
        rigs2 = {}
        cases, xs = _g_cases(rig, rigs2)
        for k in range(1, 8, 2):
            rigs2[k] = rig.up(np.stack([np.roll(xs[k][0], b, axis=1) for b in range(2)]), 2)
        ctx.sync()
        ctx.SetCoalescing(64, 3000)
        ctx.SetDeferred(deferred)
        for name, make in cases.items():
            made = [make(k) for k in range(8)]
            outs = []
            for call, want, level, init in made:
                B = 2 if np.asarray(want).ndim == 3 else 1
                outs.append(rig.out(B, init))
            ctx.sync()
            _run_threads([(lambda c=made[k][0], p=outs[k][0]: c(p)) for k in range(8)])
            ctx.sync()
            for k, (call, want, level, init) in enumerate(made):
                want = np.asarray(want)
                _check(rig, outs[k], level, want if want.ndim == 3 else want[None], f"G {name}, deferred {deferred}, caller {k}, family callers")
    finally:
        ctx.sync()
        ctx.SetDeferred(0)
        ctx.SetCoalescing(0, 0)
