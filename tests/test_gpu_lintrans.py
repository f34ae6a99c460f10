"""he_lintrans_evaluate[_many] (include/hering_lintrans.h) on the device, word for word against
oracle/circuits.py::LinTransEvaluator.EvaluateMany, at every grouping (G = 1, 2, 4 through he_lintrans_set_group) with identical
words required across G."""
import math
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import lattigo_amd as la
from drivers import lintrans as LT
from lattigo_amd import _lib
from lattigo_amd import lintrans as NL
from lattigo_amd import rlwe as R
from oracle import circuits as OC
from oracle import oracle as O
from tests import lintrans_aliasing as A
from tests.gpu_common import Pair, ctx  # noqa: F401
from tests.helpers import rng_for, uniform_poly
from tests.test_gpu_circuits import Rig, make_lt

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = (1, 2, 4)
SHAPES = [(10, [55, 45, 45, 50], [55, 46]), (12, [60, 45, 45], [61])]
SETS = [([0, 1, 2, 5], 0), ([1, 3, 130], 0), ([0, 1, 2, 3, 4, 5, 6, 7], 4), ([1, 2, 9, 17, 18], 8), ([3, 4, 5], 4)]


def native(rg, glt):
    """the library's handle over the driver transformation's own polynomials"""
    return NL.LinearTransformation(rg.gev, glt.Vec, glt.LevelQ, glt.LevelP, (0, int(math.log2(glt.slots))), glt.N1)


def rotations(diags, slots, N1):
    return list(diags) if N1 == 0 else sum(LT.BSGSIndex(diags, slots, N1)[1:], [])


def keys_for(rg, sets, slots, nth=None):
    nth = nth or 2 * rg.N
    rots = set()
    for diags, N1 in sets:
        rots |= set(rotations(diags, slots, N1))
    rg.keys([R.GaloisElement(nth, r) for r in sorted(rots) if r & (slots - 1)])


def every_group(ne, ct_level, gct, nlts, new_outs):
    """the call at G = 1, 2 and 4 into fresh outputs; the words, which must not depend on G"""
    words = None
    for G in GROUPS:
        for lt in nlts:
            lt.SetGroup(G)
        outs = new_outs()
        ne.EvaluateMany(ct_level, gct, nlts, outs)
        got = [Rig.down(o) for o in outs]
        if words is None:
            words = got
        else:
            assert all(np.array_equal(a, b) for a, b in zip(words, got)), f"G = {G} differs from G = 1"
    return words


def check_one(rg, diags, N1, triples, slots=None):
    slots = slots or rg.N // 2
    keys_for(rg, [(diags, N1)], slots)
    ne, oe = NL.Evaluator(rg.gev, rg.ggks), OC.LinTransEvaluator(rg.oev, rg.ogks)
    for ct_level, lt_level, B in triples:
        olt, glt = make_lt(rg, diags, lt_level, slots, N1)
        ct = rg.ct(ct_level, B)
        lv = min(ct_level, lt_level)
        (got,) = every_group(ne, ct_level, rg.up(ct), [native(rg, glt)], lambda: [rg.new_ct(lv, B)])
        for b in range(B):
            (want,) = oe.EvaluateMany(ct[b], [olt])
            assert np.array_equal(got[b], want), (ct_level, lt_level, b)


@pytest.mark.parametrize("logN,logq,logp", SHAPES)
@pytest.mark.parametrize("diags,N1", SETS)
def test_words_against_the_oracle(ctx, logN, logq, logp, diags, N1):
    rg = Rig(ctx, logN, logq, logp, 7300 + logN + N1 + len(diags))
    top = len(rg.q) - 1
    check_one(rg, diags, N1, ((top, top, 2), (top, top - 1, 1), (top - 1, top, 1)))


@pytest.mark.parametrize("B", [3, 5])
@pytest.mark.parametrize("diags,N1", [SETS[0], SETS[3]])
def test_batch_tails(ctx, B, diags, N1):
    """B = 3 and 5: the last block of every batch-entries-per-thread instantiation (4, 2, 1) is partly empty"""
    rg = Rig(ctx, 10, *SHAPES[0][1:], 7400 + B + N1)
    top = len(rg.q) - 1
    check_one(rg, diags, N1, ((top, top, B),))


def test_evaluate_many_mixed_and_overflow_margins(ctx):
    """61-bit moduli (the halved overflow margins trigger the intermediate Reduce calls); two BSGS transformations that share
    pre-rotations but not all of them (the second one's slot map is not the identity), one naive; the second one at a lower
    LevelQ, so the decomposition level (2) differs from its working level (1)."""
    rg = Rig(ctx, 10, [61, 61, 60], [61, 61], 7500)
    slots = rg.N // 2
    d1, d2, d3 = list(range(16)), [0, 2, 4, 6, 9, 11, 33], [1, 2, 3, 4, 5, 6, 7, 8, 9]
    keys_for(rg, [(d1, 8), (d2, 8), (d3, 0)], slots)
    ne, oe = NL.Evaluator(rg.gev, rg.ggks), OC.LinTransEvaluator(rg.oev, rg.ogks)
    o1, g1 = make_lt(rg, d1, 2, slots, 8)
    o2, g2 = make_lt(rg, d2, 1, slots, 8)
    o3, g3 = make_lt(rg, d3, 2, slots, 0)
    ct = rg.ct(2)
    got = every_group(ne, 2, rg.up(ct), [native(rg, g) for g in (g1, g2, g3)], lambda: [rg.new_ct(2), rg.new_ct(1), rg.new_ct(2)])
    wants = oe.EvaluateMany(ct[0], [o1, o2, o3])
    for k in range(3):
        assert np.array_equal(got[k][0], wants[k]), k
    with pytest.raises(ValueError):
        ne.EvaluateMany(2, rg.up(ct), [native(rg, g1), native(rg, g2)], [rg.new_ct(2)])


@pytest.mark.parametrize("diags,N1,what", [(list(range(70)), 128, "more than 64 baby steps in one giant step"),
                                           ([1, 2, 3], 4, "only j = 0"), ([0], 4, "the zero diagonal alone"),
                                           ([5, 40, 41, 72], 8, "no i = 0 term in some giant steps")])
def test_shapes_of_the_index(ctx, diags, N1, what):
    rg = Rig(ctx, 10, *SHAPES[0][1:], 7600 + len(diags))
    top = len(rg.q) - 1
    check_one(rg, diags, N1, ((top, top, 1),))


def test_logn11_below_the_fused_giant_step(ctx):
    rg = Rig(ctx, 11, [55, 45, 45], [55, 46], 7700)
    check_one(rg, SETS[3][0], SETS[3][1], ((2, 2, 2),))
    check_one(rg, SETS[0][0], SETS[0][1], ((2, 2, 1),))


class CIRig(Rig):
    """a conjugate-invariant ring (NthRoot = 4N); no oracle evaluator: the comparison is with the driver"""

    def __init__(self, ctx, logN, logq, logp, seed):
        q, p = O.GenModuli(logN + 2, logq, logp)
        self.pr = Pair(ctx, logN, len(q), len(p), qmods=q, pmods=p, ci=True)
        self.q, self.p, self.N = q, p, 1 << logN
        self.rng = rng_for(seed)
        self.gev = la.Evaluator(self.pr.gQ, self.pr.gP)
        self.beta = O.BaseRNSDecompositionVectorSize(len(q) - 1, len(p) - 1)
        self.ogks, self.ggks = {}, R.GaloisKeySet()


@pytest.mark.parametrize("diags,N1", [SETS[0], SETS[3]])
def test_conjugate_invariant_ring_against_the_driver(ctx, diags, N1):
    rg = CIRig(ctx, 10, [55, 45, 45], [55, 46], 7800 + N1)
    slots, nth = rg.N // 2, 4 * rg.N
    keys_for(rg, [(diags, N1)], slots, nth)
    ne, de = NL.Evaluator(rg.gev, rg.ggks), LT.LinTransEvaluator(rg.gev, rg.ggks)
    _, glt = make_lt(rg, diags, 2, slots, N1)
    gct = rg.up(rg.ct(2, 2))
    want = rg.new_ct(2, 2)
    de.EvaluateMany(2, gct, [glt], [want])
    (got,) = every_group(ne, 2, gct, [native(rg, glt)], lambda: [rg.new_ct(2, 2)])
    assert np.array_equal(got, Rig.down(want))


def test_galois_elements_on_both_ring_types(ctx):
    """he_lintrans_galois_elements takes NthRoot from the evaluator's ring: 2N, and 4N on a conjugate-invariant ring"""
    for rg, nth in ((Rig(ctx, 10, [55, 45], [55], 7850), 2 << 10), (CIRig(ctx, 10, [55, 45], [55], 7851), 4 << 10)):
        for diags, _ in SETS + [(list(range(-7, 8)), 0)]:
            for logr in (-1, 0, 1, 2, 3):
                assert NL.GaloisElements(rg.gev, diags, 512, logr) == LT.GaloisElements(nth, diags, 512, logr), (nth, diags, logr)
        assert NL.BSGSIndex([1, 2, 9, 17, 18], 512, 8) == LT.BSGSIndex([1, 2, 9, 17, 18], 512, 8)
        assert NL.FindBestBSGSRatio(list(range(16)), 512, 1) == LT.FindBestBSGSRatio(list(range(16)), 512, 1)


@pytest.mark.parametrize("scheme,logr", [("ckks", 1), ("ckks", -1), ("bgv", 1)])
def test_python_encode_and_evaluate_with_real_keys(ctx, scheme, logr):
    """NewLinearTransformation -> Encode (either encoder) -> EvaluateNew with generated Galois keys at logN 10: the ciphertext
    equals the oracle's on the same encoded diagonals.  CKKS also decrypts: the slots are the numpy matrix-vector product (the
    precision bound is the host test's, tests/test_lintrans_host.py: 34 bits recorded at logN 9, less its 2-bit margin and 2 more
    for the ring of twice the degree)."""
    from lattigo_amd import bgv, ckks
    from tests.rlwe_fixtures import SecretKey, ckks_decrypt, ckks_encrypt, gen_galois_keys
    logN, T = 10, 65537
    N, n = 1 << logN, 1 << (logN - 1)
    q, p = O.GenModuli(logN + 1, [55, 45, 45], [55])
    pr = Pair(ctx, logN, 3, 1, qmods=q, pmods=p)
    gev, oev = la.Evaluator(pr.gQ, pr.gP), O.Evaluator(pr.oQ, pr.oP)
    rng = np.random.default_rng(8700 + logr)
    sk = SecretKey(rng, pr.oQ, pr.oP)
    idx = [0, 1, 2, 5, 9, -3]
    if scheme == "ckks":
        encoder, dims, scale = ckks.Encoder(pr.gQ, pr.gP), (0, logN - 1), float(1 << 45)
        diagonals = {k: rng.uniform(-1, 1, n) + 0j for k in idx}
    else:
        encoder, dims, scale = bgv.Encoder(pr.gQ, la.Ring(ctx, N, [T]), pr.gP), (1, logN - 1), 1
        diagonals = {k: rng.integers(0, T, size=N, dtype=np.uint64) for k in idx}
    lt = NL.NewLinearTransformation(gev, NL.Parameters(idx, 2, 0, scale, dims, logr))
    assert (lt.N1 == 0) == (logr < 0) and sorted(lt.Vec) == sorted(k % n for k in idx)
    NL.Encode(encoder, diagonals, lt)
    galels = [g for g in lt.GaloisElements() if g != 1]
    okeys = gen_galois_keys(rng, pr.oQ, pr.oP, sk, galels)
    ne = NL.Evaluator(gev, {g: gev.NewEvaluationKey(k.q, k.p) for g, k in okeys.items()})
    olt = OC.LinearTransformation({k: (vq.download()[0], vp.download()[0]) for k, (vq, vp) in lt.Vec.items()}, 2, 0, n, lt.N1)
    z = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
    ct = ckks_encrypt(rng, pr.oQ, sk, z, scale) if scheme == "ckks" else np.stack([uniform_poly(rng, q, N) for _ in range(2)])
    gct = [la.Poly(pr.gQ, 3).upload(ct[k][None]) for k in range(2)]
    got = Rig.down(ne.EvaluateNew(2, gct, lt))[0]
    (want,) = OC.LinTransEvaluator(oev, okeys).EvaluateMany(ct, [olt])
    assert np.array_equal(got, want)
    if scheme == "ckks":
        dec = ckks_decrypt(pr.oQ, got, sk, scale * scale)
        ref = sum(d * np.roll(z, -k) for k, d in diagonals.items())
        bits = -math.log2(float(np.max(np.abs(dec - ref))))
        print(f"{scheme} logBSGSRatio {logr}: {bits:.2f} bits")
        assert bits >= 34.0 - 2.0 - 2.0, bits


@pytest.mark.parametrize("diags,N1", [SETS[0], SETS[2], SETS[3]])
def test_in_place(ctx, diags, N1):
    """n_lt = 1: every (output, input) pair of the aliasing table, and out == in as a whole"""
    rg = Rig(ctx, 10, *SHAPES[0][1:], 7900 + N1)
    slots, top = rg.N // 2, 3
    keys_for(rg, [(diags, N1)], slots)
    ne, oe = NL.Evaluator(rg.gev, rg.ggks), OC.LinTransEvaluator(rg.oev, rg.ogks)
    olt, glt = make_lt(rg, diags, top, slots, N1)
    nlt = native(rg, glt)
    ct = rg.ct(top, 2)
    want = np.stack([oe.EvaluateMany(ct[b], [olt])[0] for b in range(2)])
    names = {"in0": 0, "in1": 1}
    forms = [{o: i} for (o, i) in sorted(A.ROWS["he_lintrans_evaluate"].allowed)] + [{"out0": "in0", "out1": "in1"}, {"out0": "in1", "out1": "in0"}]
    for G in GROUPS:
        nlt.SetGroup(G)
        for form in forms:
            gct = rg.up(ct)
            out = [gct[names[form[o]]] if o in form else la.Poly(rg.pr.gQ, top + 1, 2) for o in ("out0", "out1")]
            ne.Evaluate(top, gct, nlt, out)
            assert np.array_equal(Rig.down(out), want), (G, form)


def _snapshot(polys):
    return [p.download().copy() for p in polys]


def test_rejections_leave_every_operand_unchanged(ctx):
    rg = Rig(ctx, 10, *SHAPES[0][1:], 8000)
    slots, top = rg.N // 2, 3
    d1, d2 = [0, 1, 2, 9], [0, 3, 5]
    keys_for(rg, [(d1, 4), (d2, 0)], slots)
    ne = NL.Evaluator(rg.gev, rg.ggks)
    _, g1 = make_lt(rg, d1, top, slots, 4)
    _, g2 = make_lt(rg, d2, top, slots, 0)
    n1, n2 = native(rg, g1), native(rg, g2)
    gct = rg.up(rg.ct(top))
    outs = [rg.new_ct(top), rg.new_ct(top)]
    for o in outs:
        for p in o:
            p.upload(uniform_poly(rg.rng, rg.q, rg.N)[None])
    diag = g1.Vec[1][0]
    everything = gct + outs[0] + outs[1] + [diag]
    before = _snapshot(everything)

    def rejected(call, code=-1):
        with pytest.raises(_lib.HeringError) as e:
            call()
        assert e.value.code == code, e.value
        ctx.sync()
        assert all(np.array_equal(a, b) for a, b in zip(_snapshot(everything), before))

    # operand identity: n_lt > 1 admits no output on an input; two outputs that are one polynomial; an output that is a diagonal
    for o in range(2):
        for i in range(2):
            alias = [list(outs[0]), list(outs[1])]
            alias[1][o] = gct[i]
            rejected(lambda: ne.EvaluateMany(top, gct, [n1, n2], alias))
    rejected(lambda: ne.Evaluate(top, gct, n1, [outs[0][0], outs[0][0]]))
    rejected(lambda: ne.EvaluateMany(top, gct, [n1, n2], [outs[0], [outs[1][0], outs[0][1]]]))
    rejected(lambda: ne.Evaluate(top, gct, n1, [diag, outs[0][1]]))
    # a transformation of another LevelP than the first one's
    odd = NL.LinearTransformation(rg.gev, g2.Vec, top, 0, (0, int(math.log2(slots))), 0)
    rejected(lambda: ne.EvaluateMany(top, gct, [n1, odd], outs))
    # a needed Galois element that the set does not hold
    _, g3 = make_lt(rg, [0, 1, 2, 77], top, slots, 4)
    rejected(lambda: ne.Evaluate(top, gct, native(rg, g3), outs[0]))
    # a key of another LevelP than the transformation's (the set's keys have two special primes; the transformation declares
    # LevelP = 0)
    lone = NL.LinearTransformation(rg.gev, g1.Vec, top, 0, (0, int(math.log2(slots))), 4)
    rejected(lambda: ne.Evaluate(top, gct, lone, outs[0]))
    # duplicate indices after reduction, at creation
    with pytest.raises(_lib.HeringError) as e:
        NL.LinearTransformation(rg.gev, {1: g1.Vec[1], 1 + slots: g1.Vec[2]}, top, g1.LevelP, (0, int(math.log2(slots))), 4).h
    assert e.value.code == -1
    with pytest.raises(_lib.HeringError):
        n1.SetGroup(3)
    n1.SetGroup(0)
    # too few limbs for the level, a batch mismatch
    rejected(lambda: ne.Evaluate(top, [la.Poly(rg.pr.gQ, top), gct[1]], n1, outs[0]))
    rejected(lambda: ne.Evaluate(top, gct, n1, [la.Poly(rg.pr.gQ, top + 1, 2), outs[0][1]]))


def test_base2_key_set_is_rejected(ctx):
    """the hoisted automorphisms need plain RNS digits (AutomorphismHoistedLazy panics on BaseTwoDecomposition != 0)"""
    rg = Rig(ctx, 10, [55, 45], [55], 8100)
    slots, pw2 = rg.N // 2, 16
    nj = [(int(x).bit_length() + pw2 - 1) // pw2 for x in rg.q]
    keys = {}
    for r in (1, 2):
        kq = np.stack([np.stack([uniform_poly(rg.rng, rg.q, rg.N) for _ in range(2)]) for _ in range(sum(nj))])
        kp = np.stack([np.stack([uniform_poly(rg.rng, rg.p, rg.N) for _ in range(2)]) for _ in range(sum(nj))])
        keys[R.GaloisElement(2 * rg.N, r)] = rg.gev.NewEvaluationKey(kq, kp, pw2, nj)
    ne = NL.Evaluator(rg.gev, keys)
    _, glt = make_lt(rg, [0, 1, 2], 1, slots, 0)
    gct, out = rg.up(rg.ct(1)), rg.new_ct(1)
    with pytest.raises(_lib.HeringError) as e:
        ne.Evaluate(1, gct, native(rg, glt), out)
    assert e.value.code == -1 and "BaseTwoDecomposition" in str(e.value)


def poison_case():
    """run by test_every_output_word_is_written in a process of its own with HERING_POISON=1: the outputs are scratch polynomials"""
    c = la.Context(0)
    rg = Rig(c, 10, *SHAPES[0][1:], 8200)
    slots, top = rg.N // 2, 3
    sets = [SETS[0], SETS[3], ([1, 2, 3], 4)]
    keys_for(rg, sets, slots)
    ne, oe = NL.Evaluator(rg.gev, rg.ggks), OC.LinTransEvaluator(rg.oev, rg.ogks)
    for diags, N1 in sets:
        olt, glt = make_lt(rg, diags, top, slots, N1)
        ct = rg.ct(top, 3)
        for G in GROUPS:
            nlt = native(rg, glt)
            nlt.SetGroup(G)
            out = [la.Poly(rg.pr.gQ, top + 1, 3, zero=False) for _ in range(2)]
            ne.Evaluate(top, rg.up(ct), nlt, out)
            got = Rig.down(out)
            for b in range(3):
                assert np.array_equal(got[b], oe.EvaluateMany(ct[b], [olt])[0]), (diags, G, b)
    c.sync()


def test_every_output_word_is_written(ctx):
    env = dict(os.environ, HERING_POISON="1")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c",
                        "import tests.conftest; from tests.test_gpu_lintrans import poison_case; poison_case()"],  # (conftest: the drivers' path)
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


# ---- launch census -----------------------------------------------------------------------------------------------------------------
def _prof(ctx, call):
    call()  # (plans, index tables and the arena are built on first use)
    ctx.sync()
    ctx.prof_begin()
    call()
    ctx.sync()
    return {k: v[0] for k, v in ctx.prof_end().items()}


@pytest.mark.parametrize("logN", [10, 12])
def test_launch_census(ctx, logN):
    shape = SHAPES[0] if logN == 10 else SHAPES[1]
    rg = Rig(ctx, *shape, 8300 + logN)
    slots, top = rg.N // 2, len(rg.q) - 1
    diags, N1 = [0, 1, 2, 3, 8, 9, 17, 18, 26, 35, 41], 8  # giant steps 0, 8, 16, 24, 32, 40; baby steps 0, 1, 2, 3
    keys_for(rg, [(diags, N1)], slots)
    ne, de = NL.Evaluator(rg.gev, rg.ggks), LT.LinTransEvaluator(rg.gev, rg.ggks)
    _, glt = make_lt(rg, diags, top, slots, N1)
    nlt = native(rg, glt)
    gct, out = rg.up(rg.ct(top, 2)), rg.new_ct(top, 2)
    n_giant, n_baby = 6, 3
    n = lambda d: sum(d.values())
    B, levelP = 2, len(rg.p) - 1
    # the pieces, each profiled alone on polynomials of the same shape: ONE DecomposeNTT, one AutomorphismHoistedLazy, one
    # ModDownQPtoQNTT in place, one accumulating giant step
    dec = R.Decomposition(rg.gev, B)
    qp = lambda: (la.Poly(rg.pr.gQ, top + 1, B), la.Poly(rg.pr.gP, levelP + 1, B))
    a0, a1, t0, t1 = qp(), qp(), qp(), qp()
    gal_b, gal_g = R.GaloisElement(2 * rg.N, 1), R.GaloisElement(2 * rg.N, 8)
    kb, kg = rg.ggks.GetGaloisKey(gal_b), rg.ggks.GetGaloisKey(gal_g)
    one_dec = _prof(ctx, lambda: rg.gev.DecomposeNTT(top, levelP, levelP + 1, gct[1], True, dec))
    one_auto = _prof(ctx, lambda: rg.gev.AutomorphismHoistedLazy(top, gct, dec, gal_b, kb, [a0, a1]))
    one_md = _prof(ctx, lambda: rg.gev.ModDownQPtoQNTT(top, levelP, t1[0], t1[1], t1[0]))
    one_giant = _prof(ctx, lambda: rg.gev.LinTransGiantStep(top, t1[0], kg, gal_g, t0, (a0, a1), True))
    # the Reduce calls of the outer accumulators (:443-464): after giant step c when c % over == over - 1, and at the end
    reduces = lambda over: sum(1 for c in range(n_giant) if c % over == over - 1) + (1 if n_giant % over else 0)
    overQ, overP = LT._overflow_margin(rg.q, top) >> 1, LT._overflow_margin(rg.p, levelP) >> 1
    drv = _prof(ctx, lambda: de.EvaluateMany(top, gct, [glt], [out]))
    for G in GROUPS:
        nlt.SetGroup(G)
        got = _prof(ctx, lambda: ne.Evaluate(top, gct, nlt, out))
        # exactly: one decomposition; one hoisted automorphism per distinct non-zero baby step; per giant step j != 0 the ModDown
        # of tmp1 and the giant step; the two final ModDowns; the grouped kernel per ring part and group; element-wise: P * c0 and
        # P * c1, two launches per Reduce of the Q or of the P accumulators.  Giant step 0 costs nothing beyond its group's launch.
        want = {}
        for piece, times in ((one_dec, 1), (one_auto, n_baby), (one_md, n_giant - 1 + 2), (one_giant, n_giant - 1)):
            for k, c in piece.items():
                want[k] = want.get(k, 0) + times * c
        want["diag_mac_group"] = 2 * math.ceil(n_giant / G)
        want["ew"] = want.get("ew", 0) + 2 + 2 * reduces(overQ) + 2 * reduces(overP)
        print("G", G, got, "\nwant", want, "\ndriver", drv, "\npieces", one_dec, one_auto, one_md, one_giant)
        assert got == want, (G, got, want)
        assert got.get("diag_mac", 0) == 0
        assert n(got) <= n(drv), (G, n(got), n(drv))
    # the naive form keeps the one-term kernel
    _, g0 = make_lt(rg, [0, 1, 2], top, slots, 0)
    got = _prof(ctx, lambda: ne.Evaluate(top, gct, native(rg, g0), out))
    drv0 = _prof(ctx, lambda: de.EvaluateMany(top, gct, [g0], [out]))
    assert got.get("diag_mac_group", 0) == 0 and got.get("diag_mac", 0) == 4
    assert n(got) <= n(drv0), (got, drv0)


# ---- the submission queue, graphs and replay -----------------------------------------------------------------------------------------
def _setup(ctx, seed):
    rg = Rig(ctx, 10, *SHAPES[0][1:], seed)
    slots, top = rg.N // 2, 3
    sets = [SETS[3], SETS[0]]
    keys_for(rg, sets, slots)
    ne = NL.Evaluator(rg.gev, rg.ggks)
    nlts = [native(rg, make_lt(rg, d, top, slots, N1)[1]) for d, N1 in sets]
    nlts[0].SetGroup(2)
    return rg, ne, nlts, top


@pytest.mark.parametrize("deferred", [0, 4])
def test_queue_coalesced_and_deferred(ctx, deferred):
    """8 threads on their own batch-1 handles; bit-identical to the direct calls (the requests are served one by one)"""
    rg, ne, nlts, top = _setup(ctx, 8400 + deferred)
    TH, REP = 8, 2
    ins = [rg.up(rg.ct(top)) for _ in range(TH)]
    want = []
    for t in range(TH):
        outs = [rg.new_ct(top), rg.new_ct(top)]
        ne.EvaluateMany(top, ins[t], nlts, outs)
        want.append([Rig.down(o) for o in outs])
    ctx.sync()
    outs = [[rg.new_ct(top), rg.new_ct(top)] for _ in range(TH)]
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
                    ne.EvaluateMany(top, ins[t], nlts, outs[t])
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
        for k in range(2):
            assert np.array_equal(Rig.down(outs[t][k]), want[t][k]), (t, k)
    assert s1["calls"] - s0["calls"] == TH * REP, (s0, s1)


def _two_calls(rg, ne, nlts, top, gct, outs, single):
    ne.EvaluateMany(top, gct, nlts, outs)
    ne.Evaluate(top, gct, nlts[0], single)


def _replay_setup(ctx, seed):
    rg, ne, nlts, top = _setup(ctx, seed)
    gct = rg.up(rg.ct(top))
    outs, single = [rg.new_ct(top), rg.new_ct(top)], rg.new_ct(top)
    [lt.h for lt in nlts]  # (the handles are made before a recording starts: a transformation is shared, not replayed)
    return (lambda: _two_calls(rg, ne, nlts, top, gct, outs, single)), outs[0] + outs[1] + single, (rg, ne, nlts)


def test_graph_capture_and_launch(ctx):
    run, outs, keep = _replay_setup(ctx, 8500)
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
    run, outs, keep = _replay_setup(ctx, 8600)
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
