"""The third leg of the ring-degree maps and the ring-packing kernels, without a device: the reference's sequences of calls on the
oracle (the yardstick of tests/test_gpu_ringmap_edges.py) against the closed forms that include/hering_ringswitch.h and
include/hering_ringpack.h promise, in Python integers (tests/ringmap_ref.py), on every ring, shape and family of
tests/ringmap_edges.py; and the property each planted family is built for, asserted from the integer model.

Sizes: the planted families and the row families are whole everywhere.  At N = 1024 and 2048 the closed forms of the step kernels
run over entry 0 of each batch for the row families (entries 1 and 2 are the same kinds, moved), over every entry for the planted ones."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import boundary as Bd
from tests import ringmap_edges as X
from tests import ringmap_ref as M

U = np.uint64
B = X.BATCH


def _same(got, want, what):
    got, want = np.asarray(got, dtype=U), np.asarray(want, dtype=U)
    if not np.array_equal(got, want):
        at = tuple(int(v) for v in np.argwhere(got != want)[0])
        raise AssertionError(f"{what}: oracle {int(got[at]):#x}, closed form {int(want[at]):#x} at (limb, position) {at} "
                             f"({int((got != want).sum())} words differ)")


def _entries(family, n):
    return range(B) if family in X.PLANTED + X.LAZY_PLANTED or n <= 64 else range(1)


# ---- the chains ------------------------------------------------------------------------------------------------------------------
def test_chains_have_their_classes_and_distances():
    """the mixed chains are built by boundary.class_chain, which asserts class and distance of every prime; here that they exist
    for every degree used, that neighbouring limbs differ in size both ways, and the 48 + 1 primes of the longest chain"""
    for n, gap in X.DEGREE_SHAPES:
        for ci in (False, True):
            N = n * gap
            q = X.mixed(N.bit_length() - 1, ci)
            assert list(q) == Bd.class_chain(N.bit_length() - 1 + ci, "hdIiD")
            assert all((m - 1) % ((4 if ci else 2) * N) == 0 for m in q)
            assert [Bd.modulus_class(m) for m in q] == [2, 0, 2, 1, 1]
            s = [m.bit_length() for m in q]
            assert s[0] > s[1] < s[2] > s[3] > s[4]
            O.Ring(N, q, ci), O.Ring(n, q, ci)
    q = X.chain49()
    assert len(set(q)) == 49 and all(m % 64 == 1 and O.IsPrime(m) for m in q)
    assert [Bd.modulus_class(m) for m in q[:6]] == [2, 0, 1, 2, 0, 1] and {Bd.modulus_class(m) for m in q} == {0, 1, 2}
    for c, bits in enumerate(Bd.CLASS_BITS):  # the k-th prime of a class within 2^(6 + 10) of its threshold
        assert all((1 << bits) - m < (1 << 16) for m in q if Bd.modulus_class(m) == c)
    O.Ring(32, q[:48]), O.Ring(16, q[:48])
    assert X.rings_for(32).keys() == {"mixed", "q193", "q12289"} and X.rings_for(64).keys() == {"mixed", "q12289"}
    assert X.rings_for(2048).keys() == {"mixed", "q12289"} and X.rings_for(4096).keys() == {"mixed"}
    assert X.rings_for(32, True).keys() == {"mixed", "q12289"} and X.rings_for(1024, True).keys() == {"mixed", "q12289"}


# ---- the fold ---------------------------------------------------------------------------------------------------------------------
def _fold_properties(family, a, mods, gap):
    for i, q in enumerate(mods):
        p = X.fold_arguments(a[:, i], q, gap)
        what = (family, gap, hex(q), p)
        if family == "cred":
            if gap <= 4:  # exact multiples of q (the output must be 0 and not q), and the sums beside them
                assert p["sum"] >= set(range(gap)) and p["sum_near"] == {-1, 1}, what
            else:  # acc + BRedAdd(partial) = q - 1, q, q + 1 across a trip; BRedAdd's own subtraction at equality
                assert p["acc"] == {-1, 0, 1}, what
                assert p["bred"] >= {-1, 0} and (1 in p["bred"] or q < (1 << 32)), what
        if family == "lazy_multiples" and gap <= 4:  # (the generic path meets the same four-word groups inside single trips)
            assert p["sum"] >= ({1, 2, 3} if gap == 2 else {4, 5, 6, 7}), what
        if family == "max_lazy":
            assert p["max"] == min(gap, 4) * (2 * q - 1), what


@pytest.mark.parametrize("ci", [False, True])
@pytest.mark.parametrize("n,gap", X.DEGREE_SHAPES)
def test_fold_sequence_equals_closed_form(n, gap, ci):
    N = n * gap
    for name, mods in X.rings_for(N, ci).items():
        for level in X.levels(len(mods)):
            m = list(mods[: level + 1])
            for fam in X.FOLD_FAMILIES:
                for k, a in enumerate(X.fold_inputs(fam, m, n, gap, B, 9100)):
                    assert a.shape == (B, level + 1, N) and (a.max(axis=(0, 2)) < 2 * np.array(m, dtype=U)).all()
                    if fam not in X.LAZY_ROWS + X.LAZY_PLANTED:
                        assert (a.max(axis=(0, 2)) < np.array(m, dtype=U)).all(), (fam, "canonical words")
                    if level == len(mods) - 1:
                        _fold_properties(fam, a, m, gap)
                    for b in _entries(fam, n):
                        _same(M.ref_down_ntt(a[b], m, N, gap, ci), M.fold(a[b], m, gap), f"fold {n} x {gap}, ci {ci}, ring {name}, level {level}, family {fam}, page {k}, entry {b}")


def test_lazy_bound_of_the_four_word_sum():
    """the bound ring_fold_kernel<4>'s comment rests on: at the largest prime below 2^61 four lazy words sum to 8q - 4, above 2^63
    and below 2^64 -- and the generic path's partial sums are the same four words"""
    for logN in (6, 14, 12):
        q = X.mixed(logN)[0]
        assert Bd.modulus_class(q) == 2 and (1 << 61) - q < (1 << (logN + 8))
        a = X.fold_inputs("max_lazy", [q], 16, 4, 1, 0)[0]
        s = sum(a[0, 0, :4].tolist())
        assert s == 8 * q - 4 and (1 << 63) < s < (1 << 64)
        assert X.fold_arguments(a[:, 0], q, 4)["max"] == s


# ---- split / merge ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", X.PACK_DEGREES)
def test_split_and_merge_sequences_equal_closed_forms(N):
    n = N // 2
    for name, mods in X.rings_for(N).items():
        rb = M.roots(N, tuple(mods), True)
        tw = X.merge_twiddles(N, mods)
        for level in X.levels(len(mods)):
            m = list(mods[: level + 1])
            for fam in X.CANONICAL_FAMILIES:
                tag = f"N {N}, ring {name}, level {level}, family {fam}"
                for k, a in enumerate(X.split_inputs(fam, m, N, B, 9200)):
                    assert (a.max(axis=(0, 2)) < np.array(m, dtype=U)).all()
                    if fam == "cred" and level == len(mods) - 1:
                        for i, q in enumerate(m):
                            p = X.pair_arguments("split", a[:, i, 0::2], a[:, i, 1::2], q, rb[i][n:])
                            assert p["sum"] == {-1, 0, 1} and p["dif_arg"] == {0, 1, 2} and 0 in p["mred"], (tag, hex(q), p)
                            assert p["halve"] == {("even", 0), ("even", 1), ("odd", 0), ("odd", 1)}, (tag, hex(q), p)
                    for b in _entries(fam, n):
                        ge, go = M.seq_split(a[b], m)
                        we, wo = M.split(a[b], m)
                        _same(ge, we, f"split even, {tag}, page {k}, entry {b}")
                        _same(go, wo, f"split odd, {tag}, page {k}, entry {b}")
                for k, (e, o) in enumerate(X.pair_inputs("merge", fam, m, n, B, 9300, tw)):
                    assert (e.max(axis=(0, 2)) < np.array(m, dtype=U)).all() and (o.max(axis=(0, 2)) < np.array(m, dtype=U)).all()
                    if fam == "cred" and level == len(mods) - 1:
                        for i, q in enumerate(m):
                            p = X.pair_arguments("merge", e[:, i], o[:, i], q, tw[i])
                            assert p["sum"] == {-1, 0, 1} and p["dif"] == {-1, 0, 1}, (tag, hex(q), p)
                    for b in _entries(fam, n):
                        _same(M.seq_merge(e[b], o[b], m), M.merge(e[b], o[b], m), f"merge, {tag}, page {k}, entry {b}")
                        _same(M.seq_merge(e[b], None, m), M.merge(e[b], None, m), f"merge without the odd half, {tag}, page {k}, entry {b}")


# ---- the step kernels and the tables ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", X.PACK_DEGREES)
def test_tables_are_views_of_the_twiddle_tables(N):
    logN = N.bit_length() - 1
    for name, mods in X.rings_for(N).items():
        for div in (False, True):
            for k in range(logN):
                _same(M.seq_xpow2(N, mods, k, div, len(mods)), M.xpow2(N, mods, k, div), f"xpow2 N {N}, ring {name}, k {k}, div {div}")


@pytest.mark.parametrize("N", X.PACK_DEGREES)
def test_step_sequences_equal_closed_forms(N):
    logN = N.bit_length() - 1
    for name, mods in X.rings_for(N).items():
        for level in X.levels(len(mods)):
            m = list(mods[: level + 1])
            top = level == len(mods) - 1
            for fam in X.CANONICAL_FAMILIES:
                for kk in X.table_indices(logN):
                    tag = f"N {N}, ring {name}, level {level}, family {fam}, k {kk}"
                    xinv = M.xpow2(N, mods, kk, True)
                    for pg, (a, t) in enumerate(X.pair_inputs("expand", fam, m, N, B, 9400)):
                        if fam == "cred" and top:
                            for i, q in enumerate(m):
                                p = X.pair_arguments("expand", a[:, i], t[:, i], q, xinv[i])
                                assert p["sum"] == {-1, 0, 1} and p["dif_arg"] == {0, 1, 2} and 0 in p["mred"], (tag, hex(q), p)
                        for b in _entries(fam, N):
                            for got, want, part in zip(M.seq_expand(a[b], t[b], m, kk), M.expand(a[b], t[b], m, kk), ("sum", "difference")):
                                _same(got, want, f"expand {part}, {tag}, page {pg}, entry {b}")
                    tw = X.pack_twiddles(N, mods, kk)
                    for pg, (a, bb) in enumerate(X.pair_inputs("pack_pre", fam, m, N, B, 9500 + kk, tw)):
                        if fam == "cred" and top:
                            for i, q in enumerate(m):
                                p = X.pair_arguments("pack_pre", a[:, i], bb[:, i], q, tw[i])
                                assert p["sum"] == {-1, 0, 1} and p["dif"] == {-1, 0, 1}, (tag, hex(q), p)
                        for b in _entries(fam, N):
                            for kind, (pa, pb) in (("both", (a[b], bb[b])), ("a", (a[b], None)), ("b", (None, bb[b]))):
                                for got, want, part in zip(M.seq_pack_pre(pa, pb, m, kk), M.pack_pre(pa, pb, m, kk), ("a", "b", "T")):
                                    assert (got is None) == (want is None)
                                    if got is not None:
                                        _same(got, want, f"pack pre ({kind}) {part}, {tag}, page {pg}, entry {b}")
                tag = f"N {N}, ring {name}, level {level}, family {fam}"
                for pg, (v, T) in enumerate(X.pair_inputs("pack_post", fam, m, N, B, 9600)):
                    if fam == "cred" and top:
                        for i, q in enumerate(m):
                            p = X.pair_arguments("pack_post", v[:, i], T[:, i], q)
                            assert p["sum"] == {-1, 0, 1} and p["dif"] == {-1, 0, 1}, (tag, hex(q), p)
                    for b in _entries(fam, N):
                        _same(M.seq_pack_post(v[b], None, T[b], m)[0], M.pack_post(v[b], None, T[b], m)[0], f"pack post a, {tag}, page {pg}, entry {b}")
                        _same(M.seq_pack_post(None, v[b], T[b], m)[1], M.pack_post(None, v[b], T[b], m)[1], f"pack post b, {tag}, page {pg}, entry {b}")


# ---- the longest chain ---------------------------------------------------------------------------------------------------------------
def test_the_48_limb_chain():
    """N = 32 -> 16 at 48 and 47 limbs: one form of each map, canonical and uniform words"""
    mods = list(X.chain48())
    tw = X.merge_twiddles(32, mods)
    for level in (47, 46):
        m = mods[: level + 1]
        for fam in ("cred", "canonical", "uniform"):
            for a in X.fold_inputs(fam, m, 16, 2, B, 9700):
                for b in range(B):
                    _same(M.ref_down_ntt(a[b], m, 32, 2, False), M.fold(a[b], m, 2), f"fold, 48-limb chain, level {level}, family {fam}, entry {b}")
            for a in X.split_inputs(fam, m, 32, B, 9710):
                for got, want in zip(M.seq_split(a[0], m), M.split(a[0], m)):
                    _same(got, want, f"split, 48-limb chain, level {level}, family {fam}")
            for e, o in X.pair_inputs("merge", fam, m, 16, B, 9720, tw):
                _same(M.seq_merge(e[0], o[0], m), M.merge(e[0], o[0], m), f"merge, 48-limb chain, level {level}, family {fam}")
            for a, t in X.pair_inputs("expand", fam, m, 32, B, 9730):
                for got, want in zip(M.seq_expand(a[0], t[0], m, 4), M.expand(a[0], t[0], m, 4)):
                    _same(got, want, f"expand, 48-limb chain, level {level}, family {fam}")


# ---- the layout ----------------------------------------------------------------------------------------------------------------------
def test_every_tuple_meets_both_words_of_a_pair():
    """each tuple of a planted family sits at an even and at an odd unit (the two words of a thread's 16-byte pair), at every shape"""
    q = X.mixed(10)[0]
    for units in (16, 512, 1024, 2048):
        for nt in (len(X.pair_specs("split", "canonical", q, None)), len(X.pair_specs("split", "cred", q, None)), len(X.fold_groups("cred", q, 8, None))):
            pos = X.E.positions(nt, units, B)
            j = np.broadcast_to(np.arange(units), pos.shape)
            for t in range(nt):
                assert {int(v) & 1 for v in j[pos == t]} == {0, 1}, (units, nt, t)
