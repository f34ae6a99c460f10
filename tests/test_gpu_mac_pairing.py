"""The 4096-row NTT + key-MAC kernel (`ntt_mac_f64_dma_kernel<12, ...>`) through every instantiation, every word of every batch
entry against `oracle.Evaluator` (`-m gpu`).

The kernel takes the two extension rows of an item's fused ModDown epilogue as one pair of transforms per wave (the tensor
form: EPI + TEN); its other forms run one transform at a time.  What a work item does depends on how many foreign digits it
transforms (beta - 1 for a Q limb, whose own digit is the NTT-domain input itself; beta for a P limb), on where its own digit
sits, on the batch (work list shorter than the grid; XCD swizzle or not) and on the epilogue form.  The cases:

* chains with one special prime (alpha = 1) at every level 0..5: beta = 1..6, so the count of foreign transformed digits per
  item takes each of 0, 1, 2, 3, 4, 5 and the own digit is the first, a middle and the last one (logN = 12);
* a chain with two special primes, at the top level and below it (logN = 12 and 15): the last digit is short (one limb) and
  the own digit is first, middle and last;
* a chain whose second special prime is below 2^47 (logN = 12): P-limb items, beta foreign digits each, no fused epilogue
  (the P part depends on this kernel), and GadgetProduct takes the double-format accumulators;
* batches 1 and 9 everywhere, the ragged 255 at logN = 12 (1 and 9: fewer items than workgroups; 9 and 255: odd item counts, no
  XCD swizzle); tests/test_gpu_headline.py holds the headline shape itself at 9 / 128 / 255 / 256.

Instantiations reached (template arguments LOGB, QF64, EPI, SCAT, TEN):
  GadgetProductLazy                      <12, false>                       plain accumulators (Q and P limbs)
  GadgetProduct (f64-class special prime) <12, true>                        double-format Q accumulators, read by the fused ModDown
  GadgetProduct                          <12, false, true>                  epilogue without addend
  Relinearize, ApplyEvaluationKey        <12, false, true>                  epilogue with addend(s)
  BGVMulRelin, CKKSMulRelin              <12, false, true, false, true>     epilogue forming the tensor term: the PAIRED form
  Automorphism (logN = 15)               <12, false, true, true>            epilogue storing through the automorphism
  LinTransGiantStep                      <12, false, false, true>           giant step, overwriting and accumulating
Every call is made twice on the same handles (no state between launches)."""
import numpy as np
import pytest

import lattigo_amd as la
from oracle import oracle as O
from tests.gpu_common import Pair, ctx  # noqa: F401
from tests.helpers import rng_for, uniform_poly

pytestmark = pytest.mark.gpu

T_PLAIN = 65537


class _Env:
    def __init__(self, ctx, logN, logq, logp, seed):
        self.q, self.p = O.GenModuli(logN + 1, logq, logp)
        self.q, self.p = list(self.q), list(self.p)
        self.pr = Pair(ctx, logN, len(self.q), len(self.p), qmods=self.q, pmods=self.p)
        self.N = self.pr.N
        self.rng = rng_for(seed)
        self.gev, self.oev = la.Evaluator(self.pr.gQ, self.pr.gP), O.Evaluator(self.pr.oQ, self.pr.oP)
        nq, np_ = len(self.q), len(self.p)
        self.beta = (nq + np_ - 1) // np_
        kq = np.stack([np.stack([uniform_poly(self.rng, self.q, self.N) for _ in range(2)]) for _ in range(self.beta)])
        kp = np.stack([np.stack([uniform_poly(self.rng, self.p, self.N) for _ in range(2)]) for _ in range(self.beta)])
        self.gkey, self.okey = self.gev.NewEvaluationKey(kq, kp), O.EvaluationKey(kq, kp)

    def polys(self, level, B, n):
        """n polynomials of B entries at `level`: ([n][B][level + 1][N] words, their device copies)"""
        Qm = self.q[: level + 1]
        host = [np.stack([uniform_poly(self.rng, Qm, self.N) for _ in range(B)]) for _ in range(n)]
        return host, [la.Poly(self.pr.gQ, level + 1, B).upload(h) for h in host]

    def outs(self, level, B, n=2):
        return [la.Poly(self.pr.gQ, level + 1, B) for _ in range(n)]


def _get(p, B):
    a = p.download()  # [batch][limbs][N]
    assert a.shape[0] == B
    return a


def _twice(call, outs, B, want, what):
    """the call, checked word for word on every entry, then once more on the same handles"""
    for rep in range(2):
        call()
        got = [_get(o, B) for o in outs]
        for b in range(B):
            for k in range(len(outs)):
                assert np.array_equal(got[k][b], want[b][k]), what + (rep, b, k)


def _add_mod(x, y, mods):
    out = np.empty_like(x)
    for i, m in enumerate(mods):
        s = x[i] + y[i]
        out[i] = np.where(s >= np.uint64(m), s - np.uint64(m), s)
    return out


def _key_switch_forms(e, level, B, automorphism):
    """every form of the key switch that ends in the fused epilogue or the plain accumulators, at one level and batch"""
    N, Qm, oev, gev = e.N, e.q[: level + 1], e.oev, e.gev
    tag = (int(np.log2(N)), len(e.q), len(e.p), level, B)
    (c0, c1, c2, d0, d1), (g0, g1, g2, h0, h1) = e.polys(level, B, 5)
    np_ = len(e.p)
    # GadgetProductLazy: the accumulators themselves, Q and P parts
    acc = [(la.Poly(e.pr.gQ, level + 1, B), la.Poly(e.pr.gP, np_, B)) for _ in range(2)]
    want = []
    for b in range(B):
        wQ, wP = oev.GadgetProductLazy(level, c2[b], e.okey)
        want.append([wQ[0], wP[0], wQ[1], wP[1]])
    _twice(lambda: gev.GadgetProductLazy(level, g2, e.gkey, acc), [acc[0][0], acc[0][1], acc[1][0], acc[1][1]], B, want,
           ("GadgetProductLazy",) + tag)
    # GadgetProduct: ModDown fused into the kernel (no addend), or double-format accumulators for the fused ModDown launch
    o = e.outs(level, B)
    want = [oev.GadgetProduct(level, c2[b], e.okey) for b in range(B)]
    _twice(lambda: gev.GadgetProduct(level, g2, e.gkey, o), o, B, want, ("GadgetProduct",) + tag)
    # Relinearize: both addends
    want = [oev.Relinearize(np.stack([c0[b], c1[b], c2[b]]), e.okey) for b in range(B)]
    _twice(lambda: gev.Relinearize(level, [g0, g1, g2], e.gkey, o), o, B, want, ("Relinearize",) + tag)
    # ApplyEvaluationKey, same degree: (c0 + GadgetProduct(c1)[0], GadgetProduct(c1)[1]) -- one addend
    want = []
    for b in range(B):
        gp = oev.GadgetProduct(level, c1[b], e.okey)
        want.append([_add_mod(gp[0], c0[b], Qm), gp[1]])
    _twice(lambda: gev.ApplyEvaluationKey(level, [g0, g1], e.gkey, o), o, B, want, ("ApplyEvaluationKey",) + tag)
    # MulRelin, both schemes: the tensor term in the epilogue
    want = [oev.BGVMulRelin(T_PLAIN, np.stack([c0[b], c1[b]]), np.stack([d0[b], d1[b]]), e.okey, True) for b in range(B)]
    _twice(lambda: gev.BGVMulRelin(level, T_PLAIN, [g0, g1], [h0, h1], e.gkey, o), o, B, want, ("BGVMulRelin",) + tag)
    want = [oev.CKKSMulRelin(np.stack([c0[b], c1[b]]), np.stack([d0[b], d1[b]]), e.okey, True) for b in range(B)]
    _twice(lambda: gev.CKKSMulRelin(level, [g0, g1], [h0, h1], e.gkey, o), o, B, want, ("CKKSMulRelin",) + tag)
    # squaring: the four inputs of the tensor term are two rows
    want = [oev.BGVMulRelin(T_PLAIN, np.stack([c0[b], c1[b]]), np.stack([c0[b], c1[b]]), e.okey, True) for b in range(B)]
    _twice(lambda: gev.BGVMulRelin(level, T_PLAIN, [g0, g1], [g0, g1], e.gkey, o), o, B, want, ("BGVMulRelin squaring",) + tag)
    if automorphism:
        gal = pow(5, 3, 2 * N)
        want = [oev.Automorphism(np.stack([c0[b], c1[b]]), gal, e.okey) for b in range(B)]
        _twice(lambda: gev.Automorphism(level, [g0, g1], gal, e.gkey, o), o, B, want, ("Automorphism",) + tag)
    # the giant step of a linear transformation: overwriting, then accumulating onto arbitrary 64-bit words
    gal = pow(5, 77, 2 * N)
    idx = e.pr.oQ.AutomorphismNTTIndex(gal)
    aq = np.stack([uniform_poly(e.rng, Qm, N) for _ in range(B)])
    ap = np.stack([uniform_poly(e.rng, e.p, N) for _ in range(B)])
    gaq, gap = la.Poly(e.pr.gQ, level + 1, B).upload(aq), la.Poly(e.pr.gP, np_, B).upload(ap)
    for accumulate in (False, True):
        prev = [[e.rng.integers(0, 1 << 63, size=(B, n, N), dtype=np.uint64) * np.uint64(2) + np.uint64(1) for n in (level + 1, np_)]
                for _ in range(2)]
        want = []
        for b in range(B):
            wQ, wP = oev.GadgetProductLazy(level, c2[b], e.okey)
            row = []
            for k in range(2):
                for part, (w, add, mods) in enumerate(((wQ[k], aq[b], Qm), (wP[k], ap[b], e.p))):
                    v = _add_mod(w, add, mods) if k == 0 else w
                    v = v[:, idx]
                    row.append(prev[k][part][b] + v if accumulate else v)  # ...ThenAddLazy: uint64 wrap-around, no reduction
            want.append(row)
        for rep in range(2):
            og = [(la.Poly(e.pr.gQ, level + 1, B).upload(prev[k][0]), la.Poly(e.pr.gP, np_, B).upload(prev[k][1])) for k in range(2)]
            gev.LinTransGiantStep(level, g2, e.gkey, gal, (gaq, gap), og, accumulate)
            got = [_get(p, B) for p in (og[0][0], og[0][1], og[1][0], og[1][1])]
            for b in range(B):
                for k in range(4):
                    assert np.array_equal(got[k][b], want[b][k]), ("LinTransGiantStep", accumulate) + tag + (rep, b, k)


@pytest.mark.parametrize("B", [1, 9, 255])
def test_every_foreign_digit_count_one_special_prime(ctx, B):
    """alpha = 1, levels 0..5: beta = 1..6, foreign transformed digits per item 0..5, every form (logN = 12)"""
    e = _Env(ctx, 12, [45] * 6, [55], 9100 + B)
    for level in ((5, 2, 0) if B == 255 else range(6)):
        _key_switch_forms(e, level, B, automorphism=False)


@pytest.mark.parametrize("logN,B", [(12, 1), (12, 9), (12, 255), (15, 1), (15, 9)])
def test_short_last_digit_and_own_digit_position(ctx, logN, B):
    """alpha = 2, seven Q limbs of which six double-precision: digits (2, 2, 2, 1) at the top level, (2, 2, 1) two levels below --
    the last digit short, the own digit first, middle and last; logN = 15 adds the epilogue that stores through the
    automorphism (eight 4096-rows per limb)"""
    e = _Env(ctx, logN, [55] + [45] * 6, [55, 55], 9200 + logN + B)
    for level in (6, 4):
        _key_switch_forms(e, level, B, automorphism=logN == 15)


@pytest.mark.parametrize("B", [1, 9, 255])
def test_special_prime_below_2_47(ctx, B):
    """one of the two special primes is a double-precision limb: P-limb items (beta foreign digits, no own digit), no fused
    epilogue in the kernel; GadgetProduct and the MulRelin forms go through the double-format accumulators"""
    e = _Env(ctx, 12, [45] * 4 + [55], [55, 45], 9300 + B)
    for level in (4, 2):
        _key_switch_forms(e, level, B, automorphism=False)
