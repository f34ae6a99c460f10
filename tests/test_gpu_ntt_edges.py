"""The stand-alone transforms and the fused rescale of small rings at the class-boundary primes (`-m gpu`), word for word
against the oracle.

Every scheme-level feature on small rings (the encoders, the samplers, the Encryptor, the KeyGenerator, the RGSW encryptor, the
multiparty protocols) rests on Ring.NTT / INTT and on DivRound / DivFloorByLastModulus of rings with logN <= 14.  The transform
is three kernels chosen per modulus -- ntt_rows_f64_kernel below 2^47, the correction-free ntt_rows_kernel<..., NC = true> below
2^58 (forward only), the Harvey form up to 2^61 -- each instantiated for the row sizes 2^4 .. 2^13, whose round structure
differs (rounds of at most four stages: a partial round unless the row size is a multiple of four stages; workgroups of one and
two threads at 2^4 and 2^5).  The exactness of the first two is a magnitude bound in the modulus, so the primes here are the
nearest ones on both sides of each threshold plus the smallest NTT-friendly prime there is, and the words the worst cases of
tests/boundary.py.  Case tables and input builders: tests/ntt_edges.py (checked without a GPU in tests/test_ntt_edges_host.py)."""
import numpy as np
import pytest

import lattigo_amd as la
from tests import ntt_edges as E
from tests.gpu_common import Pair, ctx  # noqa: F401

pytestmark = pytest.mark.gpu


def _each(fn, xs):
    return np.stack([fn(x) for x in xs])


def _check_batch(pr, xs, arg, levels):
    """Every transform entry on the batch `xs`, the oracle on `arg` (xs itself where it is inside the reference's domain of
    words below 2q, its residues otherwise: the public entries reduce first)."""
    g, o = pr.gQ, pr.oQ
    B, L = xs.shape[0], xs.shape[1]
    twoq = 2 * np.array(pr.q, dtype=np.uint64)[None, :, None]
    red = E.reduce_words(xs, pr.q)
    want_f, want_i = _each(o.NTT, arg), _each(o.INTT, arg)
    px, py, pz = pr.up(g, xs, B), la.Poly(g, L, B), la.Poly(g, L, B)
    g.NTT(px, py)
    assert np.array_equal(py.get(), want_f), "NTT"
    g.INTT(py, pz)
    assert np.array_equal(pz.get(), red), "INTT(NTT(x)) == Reduce(x)"
    g.NTTLazy(px, py)
    lz = py.get()
    assert np.all(lz < twoq), "NTTLazy range"
    assert np.array_equal(_each(lambda v: o.unop("Reduce", v), lz), want_f), "NTTLazy"
    g.INTT(px, py)
    assert np.array_equal(py.get(), want_i), "INTT"
    g.INTTLazy(px, py)
    lz = py.get()
    assert np.all(lz < twoq), "INTTLazy range"
    assert np.array_equal(_each(lambda v: o.unop("Reduce", v), lz), want_i), "INTTLazy"
    # in place (p2 is p1)
    pin = pr.up(g, xs, B)
    g.NTT(pin, pin)
    assert np.array_equal(pin.get(), want_f), "NTT in place"
    pin = pr.up(g, xs, B)
    g.INTT(pin, pin)
    assert np.array_equal(pin.get(), want_i), "INTT in place"
    # at a lower level the launch table splits by class inside the prefix, and the limbs above the level are not touched
    for level in levels:
        for name, want in (("NTT", want_f), ("INTT", want_i)):
            pw = pr.up(g, np.full(xs.shape, E.SENTINEL, dtype=np.uint64), B)
            getattr(g.AtLevel(level), name)(px, pw)
            got = pw.get()
            assert np.array_equal(got[:, : level + 1], want[:, : level + 1]), (name, "at level", level)
            assert np.all(got[:, level + 1:] == E.SENTINEL), (name, "above level", level)


def _check_case(ctx, case, ci, logN, levels):
    mods, x1, x2, nspec = E.transform_inputs(case)
    pr = Pair(ctx, logN, len(mods), qmods=mods, ci=ci)
    # the worst-case words, one kind per batch entry: inside the reference's domain, the oracle takes them as they are
    _check_batch(pr, x1, x1, levels)
    # the spectra of the all-(q - 1) and alternating polynomials (the inverse side's dense full-range input), then arbitrary
    # 64-bit words and 2^64 - 1 everywhere: the oracle on the residues
    _check_batch(pr, x2, E.reduce_words(x2, mods), levels)
    spec = pr.up(pr.gQ, x2[:nspec], nspec)
    pr.gQ.INTT(spec, spec)
    assert np.array_equal(spec.get(), E.reduce_words(x1[:nspec], mods)), "INTT of the spectra"


@pytest.mark.parametrize("case", E.TRANSFORM_CASES, ids=E.case_id)
def test_transforms_every_small_row_size_at_the_class_boundaries(ctx, case):
    """Nine limbs [s47, s47, s47^, s58, s58, s58^, s61, s61, floor] (^: the smallest prime at or above the threshold; floor: the
    smallest prime = 1 mod 2N or 4N, 97 .. 65537) on standard rings of logN 4 .. 14 and conjugate-invariant rings of logN 4 .. 13
    -- every row size 2^4 .. 2^12 of the three row kernels, the one- and two-stage column passes, and the forward fold of the
    conjugate-invariant ring, which hands the double-precision kernel words up to 4q at a 47-bit prime.  NTT, NTTLazy, INTT,
    INTTLazy, in place, at levels 3 and 6 into a sentinel-filled polynomial, and the round trip, on every entry of both
    batches."""
    ci, logN = case
    _check_case(ctx, case, ci, logN, (3, 6))


def test_transforms_five_column_stages_at_the_class_boundaries(ctx):
    """logN 18 (five column stages in one pass, rows of 2^13) on [s47, s47^, s58, s58^, s61] with the lazy worst cases; level 3
    is the only proper prefix of these five limbs that the level test applies to."""
    _check_case(ctx, "big", False, E.BIG_LOGN, (3,))


@pytest.mark.parametrize("case", E.DISPATCH_CASES, ids=E.case_id)
def test_row_kernel_dispatch_follows_the_class_thresholds(ctx, case):
    """Which row kernel a limb gets, read from the launch accounting (hering_debug.h: launches and bytes per kernel name) --
    the words cannot show it: a row launch has at most 13 stages, so the double-precision butterflies stay exact up to about
    2^48 (30 q < 2^53) and the correction-free ones up to about 2^59 (30 q < 2^64), and a threshold that has drifted up by a bit
    computes the same words at the primes next to it while running a kernel outside the bound its comment proves.  Prefixes
    [s47, s47, s47^], [.., s58, s58, s58^] and the whole chain: the limbs below 2^47, and only those, take the double-precision
    kernels; forward, the others split into one launch per integer class present (s58^ alone in the Harvey form at level 5);
    inverse, they share the Harvey form."""
    ci, logN = case
    mods = E.transform_chain(logN, ci)
    pr = Pair(ctx, logN, len(mods), qmods=mods, ci=ci)
    B = 2
    px, py = la.Poly(pr.gQ, len(mods), B), la.Poly(pr.gQ, len(mods), B)
    per_limb = B * pr.N * 8 * 2  # one stream in, one out
    for level in (2, 5, 8):
        nd, classes = E.expected_dispatch(mods[: level + 1])
        assert nd >= 2 and len(classes) == (1 if level == 2 else 2)
        for name, inverse in (("NTT", False), ("INTT", True)):
            ctx.prof_begin()
            getattr(pr.gQ.AtLevel(level), name)(px, py)
            prof = ctx.prof_end_bytes()
            d, i = ("ntt_rows_inv_f64", "ntt_rows_inv") if inverse else ("ntt_rows_fwd_f64", "ntt_rows_fwd")
            assert (prof[d][0], prof[d][2]) == (1, nd * per_limb), (name, level, prof)
            assert (prof[i][0], prof[i][2]) == (1 if inverse else len(classes), (level + 1 - nd) * per_limb), (name, level, prof)


@pytest.mark.parametrize("case", E.PAIRING_CASES, ids=E.pairing_id)
def test_inverse_entry_pairing_at_every_row_size(ctx, case):
    """The inverse double-precision row kernel takes two batch entries per workgroup (the second one's words in flight while
    the first is transformed) once the launch is large enough -- launch_rows:

        int iters = (!INV || logb > 12 || P[2].tprod) ? 1 : (wgs >= 6144 ? 2 : 1);
        if (iters > (int)grid.x) iters = (int)grid.x;

    with wgs = batch x limbs x rows per limb.  Three limbs at the double-precision edge and batch 2049 (6147 workgroups) at logN
    4, 5, 8, 11 -- the one- and two-thread workgroups, a full and a partial last round -- batch 1025 at logN 13 (two rows per limb:
    6150), and a conjugate-invariant ring at logN 8; odd batches, so that the last workgroup holds one entry.  logN 4 with batch 1
    and 2 stays below the threshold (the clamp to the batch would need 6144 workgroups for a batch of one, which no chain can
    give) and runs the one-thread workgroup on its own.  Worst-case words cycled over the entries; sampled entries against the oracle,
    and the forward transform back on every entry (INTT is injective, so the round trip pins the entries not compared)."""
    ci, logN, batch = case
    mods, x = E.pairing_inputs(case)
    pr = Pair(ctx, logN, len(mods), qmods=mods, ci=ci)
    px, py = la.Poly(pr.gQ, len(mods), batch).upload(x), la.Poly(pr.gQ, len(mods), batch, zero=False)
    pr.gQ.INTT(px, py)
    got = py.download()
    for b in E.pairing_sample(batch):
        assert np.array_equal(got[b], pr.oQ.INTT(x[b])), b
    pr.gQ.NTT(py, py)
    assert np.array_equal(py.download(), E.reduce_words(x, mods))


@pytest.mark.parametrize("case", E.RESCALE_CASES, ids=E.rescale_id)
def test_rescale_single_pass_rings_at_the_class_boundaries(ctx, case):
    """The descent of test_rescale_two_pass_rings_at_the_class_boundaries (tests/test_gpu_ring.py) where the transform is one
    launch each way (logN <= 12): the scalar prologue and the MRed epilogue ride on the row kernels themselves, at row sizes 2^4,
    2^5, 2^8, 2^11 and 2^12, and on conjugate-invariant rings of logN 4 and 10, whose NTT variants expose the lazy
    representative of the top limb's inverse (ci_ref_inv_* kernels); plus the coefficient-domain variants and their ...Many
    forms at the top level."""
    ci, logN, _ = case
    mods, polys = E.rescale_inputs(case)
    pr = Pair(ctx, logN, len(mods), qmods=mods, ci=ci)
    if ci:
        assert E.lazy_top_words(pr.oQ, polys) > 0  # a word at or above q_L did occur in the oracle's INTTLazy of the top limb
    E.rescale_descent(pr, polys, E.RESCALE_BATCH, ci=ci, coeff_top=True)
