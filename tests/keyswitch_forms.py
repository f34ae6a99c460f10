"""Every form of the key switch that ends in the fused ModDown epilogue or in the plain accumulators, each against
`oracle.Evaluator` word for word on every entry of the batch and twice on the same handles: the body that
tests/test_gpu_mac_pairing.py (GenModuli chains, uniform words) and tests/test_gpu_mac_boundary.py (class-boundary chains,
worst-case words) share."""
import numpy as np

import lattigo_amd as la
from oracle import oracle as O
from tests.boundary import TENSOR_CASES, tensor_inputs
from tests.gpu_common import Pair
from tests.helpers import rng_for, uniform_poly

T_PLAIN = 65537

ALL_FORMS = ("GadgetProductLazy", "GadgetProduct", "Relinearize", "ApplyEvaluationKey", "BGVMulRelin", "CKKSMulRelin", "squaring",
             "Automorphism", "LinTransGiantStep")


def _uniform_words(rng, mods, N):
    return uniform_poly(rng, mods, N)


class Env:
    """One parameter set on both sides, with one evaluation key.  The chain is GenModuli(logq, logp), or the explicit
    qmods / pmods; the key is uniform, or `key` = "max" (component 0 all q - 1 in every limb of Q and P, component 1 uniform) /
    "alt" (component 0 alternating 0 / q - 1)."""

    def __init__(self, ctx, logN, logq=None, logp=None, seed=0, qmods=None, pmods=None, key="uniform"):
        if qmods is None:
            qmods, pmods = O.GenModuli(logN + 1, logq, logp)
        self.q, self.p = list(qmods), list(pmods)
        self.pr = Pair(ctx, logN, len(self.q), len(self.p), qmods=self.q, pmods=self.p)
        self.N = self.pr.N
        self.rng = rng_for(seed)
        self.gev, self.oev = la.Evaluator(self.pr.gQ, self.pr.gP), O.Evaluator(self.pr.oQ, self.pr.oP)
        nq, np_ = len(self.q), len(self.p)
        self.beta = (nq + np_ - 1) // np_

        def comp0(mods):
            if key == "uniform":
                return uniform_poly(self.rng, mods, self.N)
            out = np.zeros((len(mods), self.N), dtype=np.uint64)
            for i, m in enumerate(mods):
                out[i, :: (1 if key == "max" else 2)] = m - 1
            return out

        assert key in ("uniform", "max", "alt")
        kq = np.stack([np.stack([comp0(self.q), uniform_poly(self.rng, self.q, self.N)]) for _ in range(self.beta)])
        kp = np.stack([np.stack([comp0(self.p), uniform_poly(self.rng, self.p, self.N)]) for _ in range(self.beta)])
        self.gkey, self.okey = self.gev.NewEvaluationKey(kq, kp), O.EvaluationKey(kq, kp)

    def polys(self, level, B, n, words=None):
        """n polynomials of B entries at `level`: ([n][B][level + 1][N] words, their device copies); words(rng, moduli, N) is
        called once per entry (uniform canonical words by default)"""
        Qm = self.q[: level + 1]
        words = words or _uniform_words
        host = [np.stack([words(self.rng, Qm, self.N) for _ in range(B)]) for _ in range(n)]
        return host, [la.Poly(self.pr.gQ, level + 1, B).upload(h) for h in host]

    def outs(self, level, B, n=2):
        return [la.Poly(self.pr.gQ, level + 1, B) for _ in range(n)]


def _get(p, B):
    a = p.download()  # [batch][limbs][N]
    assert a.shape[0] == B
    return a


def _first_diff(got, want):
    """(limb, position) of the first differing word"""
    d = np.argwhere(got != want)
    return tuple(int(v) for v in d[0]) if len(d) else None


def twice(call, outs, B, want, what):
    """the call, checked word for word on every entry, then once more on the same handles"""
    for rep in range(2):
        call()
        got = [_get(o, B) for o in outs]
        for b in range(B):
            for k in range(len(outs)):
                assert np.array_equal(got[k][b], want[b][k]), what + (rep, b, k, _first_diff(got[k][b], want[b][k]))


def add_mod(x, y, mods):
    out = np.empty_like(x)
    for i, m in enumerate(mods):
        s = x[i] + y[i]
        out[i] = np.where(s >= np.uint64(m), s - np.uint64(m), s)
    return out


def key_switch_forms(e, level, B, automorphism, forms=ALL_FORMS, ct_words=None, gp_words=None, tensor_case0=None):
    """the forms of the key switch named in `forms`, at one level and batch.

    ct_words: the word source of the ciphertext polynomials (canonical words: they are addends of the epilogue and the input
    of every key switch); gp_words: a source of its own for GadgetProduct's input (lazy words below 2q included), the
    ciphertext polynomial otherwise; tensor_case0: the inputs of the two MulRelins come from tests.boundary.tensor_inputs,
    entry b of the batch taking TENSOR_CASES[(tensor_case0 + b) mod 4], instead of being ciphertext polynomials."""
    N, Qm, oev, gev = e.N, e.q[: level + 1], e.oev, e.gev
    tag = (int(np.log2(N)), len(e.q), len(e.p), level, B)
    assert set(forms) <= set(ALL_FORMS)
    (c0, c1, c2, d0, d1), (g0, g1, g2, h0, h1) = e.polys(level, B, 5, ct_words)
    np_ = len(e.p)
    o = e.outs(level, B)
    lazy_want = {}

    def lazy_of_c2(b):  # the oracle's accumulators of c2, computed once per entry
        if b not in lazy_want:
            lazy_want[b] = oev.GadgetProductLazy(level, c2[b], e.okey)
        return lazy_want[b]

    if "GadgetProductLazy" in forms:  # the accumulators themselves, Q and P parts
        acc = [(la.Poly(e.pr.gQ, level + 1, B), la.Poly(e.pr.gP, np_, B)) for _ in range(2)]
        want = []
        for b in range(B):
            wQ, wP = lazy_of_c2(b)
            want.append([wQ[0], wP[0], wQ[1], wP[1]])
        twice(lambda: gev.GadgetProductLazy(level, g2, e.gkey, acc), [acc[0][0], acc[0][1], acc[1][0], acc[1][1]], B, want,
              ("GadgetProductLazy",) + tag)
    if "GadgetProduct" in forms:  # ModDown fused into the kernel (no addend), or double-format accumulators for the fused ModDown launch
        (cg,), (gg,) = e.polys(level, B, 1, gp_words) if gp_words else ((c2,), (g2,))
        want = [oev.GadgetProduct(level, cg[b], e.okey) for b in range(B)]
        twice(lambda: gev.GadgetProduct(level, gg, e.gkey, o), o, B, want, ("GadgetProduct",) + tag)
    if "Relinearize" in forms:  # both addends
        want = [oev.Relinearize(np.stack([c0[b], c1[b], c2[b]]), e.okey) for b in range(B)]
        twice(lambda: gev.Relinearize(level, [g0, g1, g2], e.gkey, o), o, B, want, ("Relinearize",) + tag)
    if "ApplyEvaluationKey" in forms:  # same degree: (c0 + GadgetProduct(c1)[0], GadgetProduct(c1)[1]) -- one addend
        want = []
        for b in range(B):
            gp = oev.GadgetProduct(level, c1[b], e.okey)
            want.append([add_mod(gp[0], c0[b], Qm), gp[1]])
        twice(lambda: gev.ApplyEvaluationKey(level, [g0, g1], e.gkey, o), o, B, want, ("ApplyEvaluationKey",) + tag)
    # MulRelin, both schemes: the tensor term in the epilogue
    if tensor_case0 is None or not {"BGVMulRelin", "CKKSMulRelin"} & set(forms):
        (t0, t1, u0, u1), (gt0, gt1, gu0, gu1), cases = (c0, c1, d0, d1), (g0, g1, h0, h1), ()
    else:
        cases = tuple(TENSOR_CASES[(tensor_case0 + b) % len(TENSOR_CASES)] for b in range(B))
        per_entry = [tensor_inputs(case, e.rng, Qm, N) for case in cases]
        t0, t1, u0, u1 = (np.stack([per_entry[b][k] for b in range(B)]) for k in range(4))
        gt0, gt1, gu0, gu1 = (la.Poly(e.pr.gQ, level + 1, B).upload(h) for h in (t0, t1, u0, u1))
    if "BGVMulRelin" in forms:
        want = [oev.BGVMulRelin(T_PLAIN, np.stack([t0[b], t1[b]]), np.stack([u0[b], u1[b]]), e.okey, True) for b in range(B)]
        twice(lambda: gev.BGVMulRelin(level, T_PLAIN, [gt0, gt1], [gu0, gu1], e.gkey, o), o, B, want, ("BGVMulRelin", cases) + tag)
    if "CKKSMulRelin" in forms:
        want = [oev.CKKSMulRelin(np.stack([t0[b], t1[b]]), np.stack([u0[b], u1[b]]), e.okey, True) for b in range(B)]
        twice(lambda: gev.CKKSMulRelin(level, [gt0, gt1], [gu0, gu1], e.gkey, o), o, B, want, ("CKKSMulRelin", cases) + tag)
    if "squaring" in forms:  # the four inputs of the tensor term are two rows
        want = [oev.BGVMulRelin(T_PLAIN, np.stack([c0[b], c1[b]]), np.stack([c0[b], c1[b]]), e.okey, True) for b in range(B)]
        twice(lambda: gev.BGVMulRelin(level, T_PLAIN, [g0, g1], [g0, g1], e.gkey, o), o, B, want, ("BGVMulRelin squaring",) + tag)
    if "Automorphism" in forms and automorphism:
        gal = pow(5, 3, 2 * N)
        want = [oev.Automorphism(np.stack([c0[b], c1[b]]), gal, e.okey) for b in range(B)]
        twice(lambda: gev.Automorphism(level, [g0, g1], gal, e.gkey, o), o, B, want, ("Automorphism",) + tag)
    if "LinTransGiantStep" not in forms:
        return
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
            wQ, wP = lazy_of_c2(b)
            row = []
            for k in range(2):
                for part, (w, add, mods) in enumerate(((wQ[k], aq[b], Qm), (wP[k], ap[b], e.p))):
                    v = add_mod(w, add, mods) if k == 0 else w
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
