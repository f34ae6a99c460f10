"""The third leg of the coefficient-wise ring operations, without a device: the oracle (oracle/lattigo_oracle.c, the yardstick of
tests/test_gpu_ringops_edges.py) against the Python-integer restatement of ring/vec_ops.go and ring/operations.go
(tests/ringops_ref.py), word for word, for every formula, at every modulus and on every operand family of
tests/ringops_edges.py; and the property each family is built for, asserted from the Python model.

Sizes: the 2^12 uniform tuples run through the binary and unary forms at the mixed chains of logN 10 and logN 4 (+ the 27-bit
prime), 97 and 12289; the scalar forms (nine scalars each), the 64-prime chain and the mixed chains of the other degrees take
2^8 uniform tuples -- the edge families are whole everywhere."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import arith_ref as A
from tests import ringops_edges as E
from tests import ringops_ref as F

U = np.uint64
M64 = F.M64

CHAINS = {
    "mixed10": (E.mixed_chain(10), E.N_UNIFORM), "mixed4+27": (E.mixed_chain(4, True), E.N_UNIFORM), "q97": ((E.Q97,), E.N_UNIFORM),
    "q12289": ((E.Q12289,), E.N_UNIFORM), "chain64": (E.chain64(), 1 << 8), "mixed8": (E.mixed_chain(8), 1 << 8),
    "mixed9+27": (E.mixed_chain(9, True), 1 << 8), "mixed11": (E.mixed_chain(11), 1 << 8), "ci4": (E.mixed_chain(4, ci=True), 1 << 8),
    "ci9": (E.mixed_chain(9, ci=True), 1 << 8),
}
N_SCALAR_UNIFORM = 1 << 8
ROW = 16  # the oracle's polynomials here: rows of 16 words (every modulus above is 1 mod 32)


def _rows(c):
    """[limbs][n] -> [rows][limbs][16], zero padded"""
    L, n = c.shape
    pad = (-n) % ROW
    c = np.concatenate([c, np.zeros((L, pad), dtype=U)], axis=1)
    return np.ascontiguousarray(c.reshape(L, -1, ROW).transpose(1, 0, 2)), n


def _flat(rows, n):
    return np.concatenate(list(rows), axis=1)[:, :n]


def _first(name, mods, fam, got, want, cols):
    bad = np.argwhere(got != want)
    if len(bad) == 0:
        return
    i, t = bad[0]
    ops = " ".join(f"{int(c[i, t]):#x}" for c in cols)
    raise AssertionError(f"{name} mod {mods[i]:#x} (limb {i}), family {fam}, tuple {t}: operands {ops}: oracle {int(got[i, t]):#x}, "
                         f"vec_ops.go {int(want[i, t]):#x} ({len(bad)} words differ)")


def test_word_reductions_meet_their_claims():
    """ringops_ref's modular_reduction.go sequences against the claims tests/arith_ref.py holds the device's primitives to (residue
    class, range) -- on canonical x lazy words, where those claims are stated"""
    for q in E.mixed_chain(10, True) + (E.Q97, E.Q12289):
        k = F.K(q)
        vals = E.canonical_edges(q) + E.lazy_edges(q)[:3]
        x = np.array([a for a in vals for _ in vals], dtype=U)
        y = np.array([b % q for _ in vals for b in vals], dtype=U)
        xs, ys = x.tolist(), y.tolist()
        for op, f in (("MRED_LAZY", F.MRedLazy), ("MRED", F.MRed), ("BRED_LAZY", F.BRedLazy), ("BRED", F.BRed)):
            A.check_truth(op, q, [x, y], np.array([f(a, b, k) for a, b in zip(xs, ys)], dtype=U), None)
        w = np.array(vals + E.word_edges(q), dtype=U)
        for op, f in (("BRED_ADD_LAZY", F.BRedAddLazy), ("BRED_ADD", F.BRedAdd), ("MFORM_LAZY", F.MFormLazy), ("MFORM", F.MForm),
                      ("IMFORM_LAZY", F.IMFormLazy), ("IMFORM", F.IMForm)):
            A.check_truth(op, q, [w], np.array([f(a, k) for a in w.tolist()], dtype=U), None)


@pytest.mark.parametrize("chain", list(CHAINS))
def test_oracle_equals_vec_ops_on_every_family(chain):
    """binary, unary, scalar, bigint, per-limb and double-scalar forms and the vector forms"""
    mods, n_uniform = CHAINS[chain]
    o = O.Ring(ROW, mods)
    L = len(mods)
    for fam in E.FAMILIES:
        for name in F.BINARY:
            cols = E.poly_cols(fam, mods, 5100, form=name, n_uniform=n_uniform)
            if cols is None:
                continue
            (rx, n), (ry, _), (rz, _) = (_rows(c) for c in cols)
            got = _flat([o.binop(name, rx[r], ry[r], rz[r]) for r in range(len(rx))], n)
            _first(name, mods, fam, got, F.arr(F.binop(name, mods, *cols)), cols)
        cols = E.poly_cols(fam, mods, 5200, n_uniform=n_uniform)
        if cols is None:
            continue
        (rx, n), (ry, _), (rz, _) = (_rows(c) for c in cols)
        for name in F.UNARY:
            got = _flat([o.unop(name, rx[r]) for r in range(len(rx))], n)
            _first(name, mods, fam, got, F.arr(F.unop(name, mods, cols[0])), cols[:1])
        # the vector forms: limb 0's y column is the vector every limb meets (any 64-bit word in the "wild" and "word64" families)
        vec = cols[1][0]
        rv, _ = _rows(vec[None, :])
        got = _flat([o.MulByVectorMontgomery(rx[r], rv[r, 0]) for r in range(len(rx))], n)
        _first("MulByVectorMontgomery", mods, fam, got, F.arr(F.MulByVectorMontgomery(mods, cols[0], vec)), cols)
        got = _flat([o.MulByVectorMontgomery(rx[r], rv[r, 0], rz[r]) for r in range(len(rx))], n)
        _first("MulByVectorMontgomeryThenAddLazy", mods, fam, got, F.arr(F.MulByVectorMontgomery(mods, cols[0], vec, cols[2])), cols)
    for fam in E.FAMILIES:
        for name in F.SCALAR:
            for s in E.scalars(mods):
                cols = E.poly_cols(fam, mods, 5300, form=name, scalar=s, n_uniform=min(n_uniform, N_SCALAR_UNIFORM))
                if cols is None:
                    continue
                (rx, n), _, (rz, _) = (_rows(c) for c in cols)
                got = _flat([o.scalarop(name, rx[r], s, rz[r]) for r in range(len(rx))], n)
                _first(f"{name}({s:#x})", mods, fam, got, F.arr(F.scalarop(name, mods, cols[0], s, cols[2])), cols)
    for fam in E.EDGE_FAMILIES + ("uniform", "wild"):
        cols = E.poly_cols(fam, mods, 5400, n_uniform=min(n_uniform, N_SCALAR_UNIFORM))
        (rx, n), _, (rz, _) = (_rows(c) for c in cols)
        for s in E.bigint_scalars(mods):
            for name in ("AddScalarBigint", "SubScalarBigint", "MulScalarBigint"):
                got = _flat([getattr(o, name)(rx[r], s) for r in range(len(rx))], n)
                _first(f"{name}({s:#x})", mods, fam, got, F.arr(F.bigintop(name, mods, cols[0], s)), cols[:1])
            got = _flat([o.MulScalarBigintThenAdd(rx[r], s, rz[r]) for r in range(len(rx))], n)
            _first(f"MulScalarBigintThenAdd({s:#x})", mods, fam, got, F.arr(F.bigintop("MulScalarBigintThenAdd", mods, cols[0], s, cols[2])), cols)
        for sc in E.rns_scalars(mods):
            got = _flat([o.MulRNSScalarMontgomery(rx[r], sc) for r in range(len(rx))], n)
            _first("MulRNSScalarMontgomery", mods, fam, got, F.arr(F.MulRNSScalarMontgomery(mods, cols[0], sc)), cols[:1])
        # the double-scalar forms switch scalar at N/2 of a row: held on whole rows of 16 words
        for s0, s1 in E.double_scalars(mods)[:: max(1, L // 8 + 1)]:
            for name in F.DOUBLE:
                acc = name.endswith("ThenAdd")
                for r in range(min(len(rx), 8)):
                    got = getattr(o, name)(rx[r], s0, s1, rz[r]) if acc else getattr(o, name)(rx[r], s0, s1)
                    want = F.arr(F.doubleop(name, mods, rx[r], s0, s1, rz[r] if acc else None))
                    _first(name, mods, fam, got, want, (rx[r], rz[r]))


def _presum(form, x, y, z, k, scalar=None):
    """the argument of the form's final CRed"""
    lazy = {"Add": "AddLazy", "Sub": "SubLazy", "MulCoeffsBarrettThenAdd": "MulCoeffsBarrettThenAddLazy",
            "MulCoeffsMontgomeryThenAdd": "MulCoeffsMontgomeryThenAddLazy", "MulCoeffsMontgomeryThenSub": "MulCoeffsMontgomeryThenSubLazy"}
    if form in lazy:
        return F.BINARY[lazy[form]](x, y, z, k)
    s = F.SCALAR[form][0](scalar, k)
    if form == "AddScalar":
        return (x + s) & M64
    if form == "SubScalar":
        return (x + k.q - s) & M64
    return (z + F.MRed(x, s, k)) & M64


@pytest.mark.parametrize("chain", ["mixed10", "mixed4+27", "q97", "q12289", "chain64"])
def test_families_have_the_property_they_are_built_for(chain):
    mods, _ = CHAINS[chain]
    for i, q in enumerate(mods):
        k = F.K(q)
        # each conditional subtraction on a sum: not taken (q - 1), equality (q), taken (q + 1)
        for form in E.CRED_FORMS:
            x, y, z = (c.tolist() for c in E.cols("cred", q, 5100 + 17 * i, form))
            assert {_presum(form, a, b, c, k) - q for a, b, c in zip(x, y, z)} == {-1, 0, 1}, (form, q)
        for form in E.CRED_SCALAR_FORMS:
            for s in E.scalars(mods):
                x, y, z = (c.tolist() for c in E.cols("cred", q, 5300 + 17 * i, form, s))
                assert {_presum(form, a, b, c, k, s) - q for a, b, c in zip(x, y, z)} == {-1, 0, 1}, (form, q, s)
        # each lazy accumulator: no wrap, a wrap to exactly 0, a wrap to 1
        for form in E.WRAP_FORMS:
            x, y, z = (c.tolist() for c in E.cols("wrap", q, 5100 + 17 * i, form))
            assert {c + E.term(form, a, b, q) - (1 << 64) for a, b, c in zip(x, y, z)} == {-1, 0, 1}, (form, q)
            assert {F.BINARY[form](a, b, c, k) for a, b, c in zip(x, y, z)} == {M64, 0, 1}, (form, q)
        # the conditional subtraction inside the reductions, on the edge families: not taken, taken, and equality
        # (MRedLazy = q: a zero product; BRedLazy / BRedAddLazy / MFormLazy = q: an operand q; IMFormLazy = q - mulhi(.., q) never
        # exceeds q: its subtraction is taken at equality alone, on a zero word)
        x, y = [], []
        for fam in E.EDGE_FAMILIES + ("uniform", "wild"):  # (a Barrett word above q at a small modulus takes 64-bit operands)
            cx, cy, _ = E.cols(fam, q, 0, n_uniform=1 << 10)
            x += cx.tolist()
            y += cy.tolist()
        for name, lazy in (("MRed", [F.MRedLazy(a, b, k) for a, b in zip(x, y)]), ("BRed", [F.BRedLazy(a, b, k) for a, b in zip(x, y)]),
                           ("BRedAdd", [F.BRedAddLazy(a, k) for a in x]), ("MForm", [F.MFormLazy(a, k) for a in x]),
                           ("IMForm", [F.IMFormLazy(a, k) for a in x])):
            assert min(lazy) < q and q in lazy and (max(lazy) > q or name == "IMForm"), (name, q, min(lazy) < q, max(lazy) > q, q in lazy)


@pytest.mark.parametrize("N,B", [(16, 1), (16, 3), (512, 2), (1024, 3)])
def test_every_edge_value_meets_both_words_of_a_pair(N, B):
    """... and, at N = 1024, both workgroups of a row; the first and the last pair of a row hold family words like the rest"""
    q = E.mixed_chain(10)[0]
    for fam in E.EDGE_FAMILIES + ("cred", "wrap"):
        form = {"cred": "Add", "wrap": E.WRAP_FORMS[0]}.get(fam)
        n = len(E.cols(fam, q, 0, form)[0])
        pos = E.positions(n, N, B)
        j = np.broadcast_to(np.arange(N), pos.shape)
        for t in range(n):
            at = j[pos == t]
            assert {int(v) & 1 for v in at} == {0, 1}, (fam, t)
            if N == 1024:
                assert {int(v) // 512 for v in at} == {0, 1}, (fam, t)
        cols = tuple(np.stack([c]) for c in E.cols(fam, q, 0, form))
        pages = E.lay(cols, N, B)
        assert len(pages) == pos.shape[0]
        for k, page in enumerate(pages):
            for c, col in zip(page, cols):
                assert c.shape == (B, 1, N) and np.array_equal(c[:, 0], col[0][pos[k]])


@pytest.mark.parametrize("N", [16, 512])
def test_permutations_match_the_reference_and_meet_every_sign_case(N):
    logN = N.bit_length() - 1
    mods = E.mixed_chain(logN, N == 16)
    o = O.Ring(N, mods)
    x = E.permutation_operand(mods, N, 5500)
    zero = x == 0
    assert zero.any(axis=1).all()
    seen = set()
    for k in E.shifts(N):
        assert np.array_equal(o.Shift(x, k), F.arr(F.Shift(x, k))), ("Shift", k)
        assert np.array_equal(o.MultByMonomial(x, k), F.arr(F.MultByMonomial(mods, x, k))), ("MultByMonomial", k)
        sh = (k + 2 * N) % (2 * N)
        if sh:
            flip, s = sh >= N, sh % N
            src0 = np.where(zero[0])[0]
            seen |= {(flip, bool(j >= N - s)) for j in src0}  # (source j lands in the wrapped part when j >= N - s)
    assert seen == {(False, False), (False, True), (True, False), (True, True)}, seen
    acc = E.cols("wild", mods[0], 5600, n_uniform=N)[2]
    acc = np.stack([acc + U(i) for i in range(len(mods))])
    for ci in (False, True):
        cm = E.mixed_chain(logN, N == 16, ci=True) if ci else mods
        oc = O.Ring(N, cm, conjugate_invariant=True) if ci else o
        xc = E.permutation_operand(cm, N, 5500)
        signs = set()
        for g in E.galois_elements(N):
            got = oc.Automorphism(xc, g)
            assert np.array_equal(got, F.arr(F.Automorphism(cm, xc, g, ci))), ("Automorphism", ci, g)
            signs |= {bool(neg) for _, src, neg in F.AutomorphismMap(N, g, ci) if xc[0, src] == 0}  # a zero word under each sign
            if ci:  # (the NTT index table of a conjugate-invariant ring stays below N only for elements = 1 mod 4: the gather is
                continue  # held on the standard ring)
            idx = oc.AutomorphismNTTIndex(g)
            assert idx.tolist() == F.AutomorphismNTTIndex(N, oc.NthRoot(), g), ("AutomorphismNTTIndex", ci, g)
            assert np.array_equal(oc.AutomorphismNTTWithIndex(xc, idx), F.arr(F.AutomorphismNTTWithIndex(xc, idx))), (ci, g)
            assert np.array_equal(oc.AutomorphismNTTWithIndexThenAddLazy(xc, idx, acc), F.arr(F.AutomorphismNTTWithIndex(xc, idx, acc))), (ci, g)
        assert signs == {True, False}, (ci, signs)
    # the gather's accumulator wraps and does not wrap
    s = (acc.astype(object) + x.astype(object))
    assert (s >= (1 << 64)).any() and (s < (1 << 64)).any()


def test_scalars_cover_what_they_are_listed_for():
    mods = E.mixed_chain(4)
    s = E.scalars(mods)
    assert any(v >= mods[0] for v in s) and any(v % mods[0] == 0 and v for v in s) and mods[-1] in s and M64 in s
    b = E.bigint_scalars(mods)
    p = 1
    for q in mods:
        p *= q
    assert p in b and any(v < 0 for v in b) and any(v < 0 and v % mods[0] == 0 for v in b) and any(v.bit_length() > 256 for v in b)
    for s0, s1 in E.double_scalars(mods):
        assert (s0 != s1).all()
    words = np.stack(E.rns_scalars(mods))
    for i, q in enumerate(mods):
        assert set(words[:, i].tolist()) == {0, q - 1, q, M64}
