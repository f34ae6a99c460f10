"""include/hering_ckks_evaluator.h on the device: the four entries word for word against tests/ckks_evaluator_ref.py (the
reference's sequences over the oracle's ring primitives, and plain arithmetic) on the pre-call words, and against the composed
sequence of the ring-level entries a caller had before (the driver leg); every aliasing form of tests/ckks_evaluator_aliasing.py;
the launch census from the profiler names; the queue, deferred submission, graph capture and replay.

Rings: logN 4 (N = 16: a partly filled block, the N/2 boundary inside one wave), logN 10 (two blocks per limb), logN 12 for the
key-switch entry.  Chains of 1, 2 and 3 limbs: the largest prime below 2^61, a 36-bit prime, the smallest prime above 2^58."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd import _lib
from lattigo_amd import ckks as K
from oracle import oracle as O
from tests import boundary as Bd
from tests import ckks_evaluator_aliasing as A
from tests import ckks_evaluator_ref as REF
from tests.gpu_common import ctx  # noqa: F401
from tests.helpers import rng_for, uniform_poly

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("uniform", "zero", "max", "uniform")
SCALARS = ("uniform", "max", "zero", "one")


def chain(logN, n):
    return [Bd.class_chain(logN, "h")[0], Bd.primes_below(36, logN + 1, 1)[0], Bd.class_chain(logN, "I")[0]][:n]


def words(kind, rng, mods, N):
    if kind == "zero":
        return np.zeros((len(mods), N), dtype=np.uint64)
    return np.stack([Bd.word_row(kind, rng, m, N) for m in mods])


def residues(kind, rng, mods):
    pick = {"uniform": lambda m: int(rng.integers(0, m)), "max": lambda m: m - 1, "zero": lambda m: 0, "one": lambda m: 1}[kind]
    return np.array([pick(int(m)) for m in mods], dtype=np.uint64)


class Case:
    def __init__(self, ctx, logN, nl, B, seed, poison=False):
        self.q, self.N, self.B, self.top = chain(logN, nl), 1 << logN, B, nl - 1
        self.g, self.o = la.Ring(ctx, self.N, self.q), O.Ring(self.N, self.q)
        self.rng, self.k, self.poison, self.ctx = rng_for(seed), 0, poison, ctx

    def levels(self):
        return [self.top] if self.top == 0 else [self.top, self.top - 1]

    def ct(self, n, B=None):
        """n components of the handle's full height: ([la.Poly], [B][n][limbs][N])"""
        B = self.B if B is None else B
        w = np.empty((B, n, len(self.q), self.N), dtype=np.uint64)
        for b in range(B):
            for c in range(n):
                w[b, c] = words(KINDS[self.k % len(KINDS)], self.rng, self.q, self.N)
                self.k += 1
        return [la.Poly(self.g, len(self.q), B).upload(np.ascontiguousarray(w[:, c])) for c in range(n)], w

    def fresh(self, n):
        return [la.Poly(self.g, len(self.q), self.B, zero=not self.poison) for _ in range(n)]

    def scal(self, level):
        kind = SCALARS[self.k % len(SCALARS)]
        self.k += 1
        return residues(kind, self.rng, self.q[: level + 1])


def down(polys, level):
    return np.stack([p.download()[:, : level + 1] for p in polys], axis=1)  # [B][n][level + 1][N]


def same(got, want_per_entry, tag):
    for b, want in enumerate(want_per_entry):
        assert np.array_equal(got[b], np.stack(want)), (tag, b)


def pick(w, b, B1=False):
    return list(w[0 if B1 else b])


# ---- the composed sequences: the ring-level entries a caller had before these (the driver leg) ---------------------------------------
def composed_add(c, level, sub, p0, p1, scaled, ratio):
    r = c.g.AtLevel(level)
    t = [list(p0), list(p1)]
    if scaled:
        tmp = c.fresh(len(t[scaled - 1]))
        for x, y in zip(t[scaled - 1], tmp):
            r.MulDoubleRNSScalar(x, ratio, ratio, y)
        t[scaled - 1] = tmp
    lo = min(len(p0), len(p1))
    out = c.fresh(max(len(p0), len(p1)))
    for i in range(lo):
        r.binop("Sub" if sub else "Add", t[0][i], t[1][i], out[i])
    for i in range(lo, len(out)):
        src = t[0][i] if len(p0) > len(p1) else t[1][i]
        out[i].CopyLvl(level, src)
        if sub and len(p1) > len(p0):
            r.unop("Neg", out[i], out[i])
    return out


# ---- he_ckks_add -------------------------------------------------------------------------------------------------------------------------
SHAPES = [(4, 1, 1), (4, 3, 3), (10, 2, 2), (10, 3, 1)]


@pytest.mark.parametrize("logN,nl,B", SHAPES)
def test_add_every_degree_pair_and_scaling(ctx, logN, nl, B):
    """degrees 0 / 1 / 2 mixed (the copy and negate tails), scaled 0 / 1 / 2, Add and Sub, the top level and one below; an op1 of
    batch 1 against the batch; words uniform, zero and q - 1 in turn, ratio words uniform, q - 1, 0 and 1 in turn"""
    c = Case(ctx, logN, nl, B, 12000 + 7 * logN + nl)
    for level in c.levels():
        r = c.g.AtLevel(level)
        for n0 in (1, 2, 3):
            for n1 in (1, 2, 3):
                for scaled in (0, 1, 2):
                    for sub in (False, True):
                        b1 = B > 1 and (n0 + n1 + scaled) % 3 == 0  # op1 broadcast
                        p0, w0 = c.ct(n0)
                        p1, w1 = c.ct(n1, 1 if b1 else B)
                        ratio = c.scal(level) if scaled else None
                        out = c.fresh(max(n0, n1))
                        K.ct_add(r, p0, p1, out, sub=sub, scaled=scaled, ratio=ratio)
                        got = down(out, level)
                        tag = (level, n0, n1, scaled, sub, b1)
                        same(got, [REF.ckks_add(c.o, level, sub, pick(w0, b), pick(w1, b, b1), scaled, ratio) for b in range(B)], tag)
                        if logN == 4:
                            same(got, [REF.exact_add(c.o, level, sub, pick(w0, b), pick(w1, b, b1), scaled, ratio) for b in range(B)], tag)
                        if not b1 and sub == bool(n0 % 2):
                            assert np.array_equal(got, down(composed_add(c, level, sub, p0, p1, scaled, ratio), level)), tag
                        assert np.array_equal(down(p0, c.top), w0) and np.array_equal(down(p1, c.top), w1), tag


def test_add_negates_a_zero_to_the_modulus_as_the_reference(ctx):
    """the one non-canonical word the header states: a component that Sub only negates holds q - x, q for x = 0"""
    c = Case(ctx, 4, 2, 1, 12100)
    p0 = [la.Poly(c.g, 2, 1)]
    p1 = [la.Poly(c.g, 2, 1), la.Poly(c.g, 2, 1)]
    out = c.fresh(2)
    K.ct_add(c.g, p0, p1, out, sub=True)
    got = down(out, 1)
    assert np.all(got[0, 0] == 0) and all(np.all(got[0, 1, i] == c.q[i]) for i in range(2))


def _alias_forms(n_out, pools):
    """every way to take each output from the inputs of its own pool position or a fresh polynomial: (index into pool | None)"""
    import itertools
    opts = [None] + list(range(len(pools)))
    for choice in itertools.product(opts, repeat=n_out):
        used = [x for x in choice if x is not None]
        if len(used) == len(set(used)):
            yield choice


def test_add_every_aliasing_form(ctx):
    """any output may be any input (in place and crossed); two outputs that are one polynomial are refused and change nothing"""
    assert A.ROWS["he_ckks_add"].allowed == {("out", "op0"), ("out", "op1")}
    c = Case(ctx, 10, 2, 2, 12200)
    level, r = 1, c.g
    for n0, n1, scaled, sub in ((2, 2, 1, False), (2, 3, 2, True), (3, 1, 0, True), (1, 2, 1, True)):
        n_out = max(n0, n1)
        ratio = c.scal(level) if scaled else None
        _, w0 = c.ct(n0)
        _, w1 = c.ct(n1)
        want = [REF.ckks_add(c.o, level, sub, list(w0[b]), list(w1[b]), scaled, ratio) for b in range(c.B)]
        for choice in _alias_forms(n_out, [0] * (n0 + n1)):
            p0 = [la.Poly(c.g, 2, c.B).upload(np.ascontiguousarray(w0[:, i])) for i in range(n0)]
            p1 = [la.Poly(c.g, 2, c.B).upload(np.ascontiguousarray(w1[:, i])) for i in range(n1)]
            pool = p0 + p1
            out = [la.Poly(c.g, 2, c.B) if x is None else pool[x] for x in choice]
            K.ct_add(r, p0, p1, out, sub=sub, scaled=scaled, ratio=ratio)
            same(down(out, level), want, (n0, n1, scaled, sub, choice))
    # op0 and op1 one ciphertext, and the output too: x + x, x - r x
    p, w = c.ct(2)
    ratio = c.scal(level)
    K.ct_add(r, p, p, p, sub=True, scaled=2, ratio=ratio)
    same(down(p, level), [REF.ckks_add(c.o, level, True, list(w[b]), list(w[b]), 2, ratio) for b in range(c.B)], "x - r x in place")
    # refusals
    p0, w0 = c.ct(2)
    p1, w1 = c.ct(2)
    o = c.fresh(2)
    everything = p0 + p1 + o
    before = [x.download().copy() for x in everything]

    def rejected(call, code=-1):
        with pytest.raises(_lib.HeringError) as e:
            call()
        assert e.value.code == code, e.value
        ctx.sync()
        assert all(np.array_equal(x.download(), y) for x, y in zip(everything, before))

    rejected(lambda: K.ct_add(r, p0, p1, [o[0], o[0]]))
    rejected(lambda: K.ct_add(r, p0, p1, [p0[0], p0[0]]))
    rejected(lambda: K.ct_add(r, p0, p1, o[:1]))
    rejected(lambda: K.ct_add(r, p0, p1, o, scaled=1))                                    # no ratio
    rejected(lambda: K.ct_add(r, p0, p1, o, scaled=3, ratio=c.scal(level)))
    rejected(lambda: K.ct_add(r, p0, p1, o, scaled=1, ratio=np.array(c.q, dtype=np.uint64)))  # a word that is its modulus
    rejected(lambda: K.ct_add(r, p0, p1, [o[0], la.Poly(c.g, 1, c.B)]))                   # too few limbs
    rejected(lambda: K.ct_add(r, p0, p1, [o[0], la.Poly(c.g, 2, c.B + 1)]))               # another batch
    rejected(lambda: K.ct_add(r, p0 + p0, p1, o + o))                                     # four components


# ---- he_ckks_scalar ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logN,nl,B", SHAPES)
def test_scalar_forms(ctx, logN, nl, B):
    c = Case(ctx, logN, nl, B, 12300 + 7 * logN + nl)
    ops = ("AddDoubleRNSScalar", "SubDoubleRNSScalar", "MulDoubleRNSScalar", "MulDoubleRNSScalarThenAdd")
    for level in c.levels():
        r = c.g.AtLevel(level)
        for n in (1, 2, 3):
            for op in (0, 1, 2, 3):
                for pre_on in ((False, True) if op == 3 else (False,)):
                    for inplace in (False, True):
                        p0, w0 = c.ct(n)
                        s0, s1 = c.scal(level), c.scal(level)
                        pre = c.scal(level) if pre_on else None
                        if op == 3:
                            out, wo = (p0, w0) if inplace else c.ct(n)
                        else:
                            out, wo = (p0 if inplace else c.fresh(n)), None
                        K.ct_scalar(r, op, p0, s0, s1, out, pre=pre)
                        got = down(out, level)
                        tag = (level, n, op, pre_on, inplace)
                        ref = lambda f: [f(c.o, level, op, list(w0[b]), s0, s1, None if wo is None else list(wo[b]), pre) for b in range(B)]
                        same(got, ref(REF.ckks_scalar), tag)
                        if logN == 4:
                            same(got, ref(REF.exact_scalar), tag)
                        if not inplace and not pre_on:  # the composed sequence: one launch per component (and a copy for the others)
                            q0, _ = [la.Poly(c.g, nl, B).upload(np.ascontiguousarray(w0[:, i])) for i in range(n)], None
                            o2 = [la.Poly(c.g, nl, B).upload(np.ascontiguousarray(wo[:, i])) for i in range(n)] if op == 3 else c.fresh(n)
                            for i in range(n):
                                if op < 2 and i:
                                    o2[i].CopyLvl(level, q0[i])
                                else:
                                    getattr(r, ops[op])(q0[i], s0, s1, o2[i])
                            assert np.array_equal(got, down(o2, level)), tag
    # crossed: out = (op0_1, op0_0)
    p0, w0 = c.ct(2)
    s0, s1 = c.scal(c.top), c.scal(c.top)
    K.ct_scalar(c.g, 2, p0, s0, s1, [p0[1], p0[0]])
    same(down([p0[1], p0[0]], c.top), [REF.ckks_scalar(c.o, c.top, 2, list(w0[b]), s0, s1) for b in range(B)], "crossed")
    everything = p0
    before = [x.download().copy() for x in everything]
    for bad in (lambda: K.ct_scalar(c.g, 2, p0, s0, s1, [p0[0], p0[0]]), lambda: K.ct_scalar(c.g, 2, p0, s0, s1, p0, pre=s0),
                lambda: K.ct_scalar(c.g, 4, p0, s0, s1, p0), lambda: K.ct_scalar(c.g, 0, p0, np.array(c.q, dtype=np.uint64), s1, p0)):
        with pytest.raises(_lib.HeringError) as e:
            bad()
        assert e.value.code == -1
        ctx.sync()
        assert all(np.array_equal(x.download(), y) for x, y in zip(everything, before))
    assert A.ROWS["he_ckks_scalar"].allowed == {("out", "op0")}


# ---- he_ckks_mul_pt ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logN,nl,B", SHAPES)
def test_mul_pt_forms(ctx, logN, nl, B):
    """a plaintext of batch 1 against the batch; then_add with and without the scale-up of the accumulator; in place"""
    c = Case(ctx, logN, nl, B, 12400 + 7 * logN + nl)
    for level in c.levels():
        r = c.g.AtLevel(level)
        for n in (1, 2, 3):
            for then_add, pre_on in ((False, False), (True, False), (True, True)):
                for b1 in ((False, True) if B > 1 else (False,)):
                    for inplace in (False, True):
                        p0, w0 = c.ct(n)
                        (pt,), wp = c.ct(1, 1 if b1 else B)
                        pre = c.scal(level) if pre_on else None
                        out, wo = (p0, w0) if inplace else (c.ct(n) if then_add else (c.fresh(n), None))
                        K.ct_mul_pt(r, p0, pt, out, then_add=then_add, pre=pre)
                        got = down(out, level)
                        tag = (level, n, then_add, pre_on, b1, inplace)
                        ref = lambda f: [f(c.o, level, list(w0[b]), wp[0 if b1 else b, 0], None if not then_add else list(wo[b]), pre) for b in range(B)]
                        same(got, ref(REF.ckks_mul_pt), tag)
                        if logN == 4:
                            same(got, ref(REF.exact_mul_pt), tag)
                        if not inplace and not pre_on:  # composed: MForm into a temporary, then a product per component
                            tmp = c.fresh(1)[0] if not b1 else la.Poly(c.g, nl, 1)
                            r.unop("MForm", pt, tmp)
                            o2 = [la.Poly(c.g, nl, B).upload(np.ascontiguousarray(wo[:, i])) for i in range(n)] if then_add else c.fresh(n)
                            q0 = [la.Poly(c.g, nl, B).upload(np.ascontiguousarray(w0[:, i])) for i in range(n)]
                            for i in range(n):
                                r.binop("MulCoeffsMontgomeryThenAdd" if then_add else "MulCoeffsMontgomery", q0[i], tmp, o2[i])
                            assert np.array_equal(got, down(o2, level)), tag
    # the output is the plaintext, and crossed components
    p0, w0 = c.ct(2)
    (pt,), wp = c.ct(1)
    K.ct_mul_pt(c.g, p0, pt, [pt, p0[0]])
    same(down([pt, p0[0]], c.top), [REF.ckks_mul_pt(c.o, c.top, list(w0[b]), wp[b, 0]) for b in range(B)], "out is pt")
    with pytest.raises(_lib.HeringError):
        K.ct_mul_pt(c.g, p0, pt, p0, pre=c.scal(c.top))
    with pytest.raises(_lib.HeringError):
        K.ct_mul_pt(c.g, p0, pt, [p0[0], p0[0]])
    assert A.ROWS["he_ckks_mul_pt"].allowed == {("out", "ct"), ("out", "pt")}


# ---- he_ckks_mul_relin_then_add ----------------------------------------------------------------------------------------------------------
class KsCase:
    """(Q | P) with random key words (arithmetic parity only) on both sides"""

    def __init__(self, ctx, logN, q, p, seed):
        self.N, self.q, self.p = 1 << logN, q, p
        self.rng = rng_for(seed)
        self.gQ, self.gP = la.Ring(ctx, self.N, q), la.Ring(ctx, self.N, p)
        self.oQ, self.oP = O.Ring(self.N, q), O.Ring(self.N, p)
        self.gev, self.oev = la.Evaluator(self.gQ, self.gP), O.Evaluator(self.oQ, self.oP)
        beta = O.BaseRNSDecompositionVectorSize(len(q) - 1, len(p) - 1)
        kq = np.stack([np.stack([uniform_poly(self.rng, q, self.N) for _ in range(2)]) for _ in range(beta)])
        kp = np.stack([np.stack([uniform_poly(self.rng, p, self.N) for _ in range(2)]) for _ in range(beta)])
        self.ork, self.grk = O.EvaluationKey(kq, kp), self.gev.NewEvaluationKey(kq, kp)

    def ct(self, n, B):
        w = np.stack([np.stack([uniform_poly(self.rng, self.q, self.N) for _ in range(n)]) for _ in range(B)])
        return [la.Poly(self.gQ, len(self.q), B).upload(np.ascontiguousarray(w[:, i])) for i in range(n)], w


def _prof(ctx, call):
    call()
    ctx.sync()
    ctx.prof_begin()
    call()
    ctx.sync()
    return {k: v[0] for k, v in ctx.prof_end().items() if v[0]}


@pytest.mark.parametrize("logN,B", [(4, 3), (10, 2)])
def test_mul_then_add_without_a_key(ctx, logN, B):
    c = Case(ctx, logN, 3, B, 12500 + logN)
    ks = la.Evaluator(c.g, None)  # (the entry addresses an evaluator; without a key no special prime is touched)
    for level in c.levels():
        for pre_on in (False, True):
            a, wa = c.ct(2)
            b, wb = c.ct(2)
            out, wo = c.ct(3)
            pre = c.scal(level) if pre_on else None
            K.ct_mul_relin_then_add(ks, level, a, b, None, out, pre=pre)
            got = down(out, level)
            args = lambda e: (c.o, level, list(wa[e]), list(wb[e]), list(wo[e]), pre)
            same(got, [REF.ckks_mul_relin_then_add(*args(e)) for e in range(B)], (level, pre_on))
            same(got, [REF.exact_mul_then_add(*args(e)) for e in range(B)], (level, pre_on))
            if not pre_on:  # composed: MForm twice, four MulCoeffsMontgomeryThenAdd
                r = c.g.AtLevel(level)
                o2 = [la.Poly(c.g, 3, B).upload(np.ascontiguousarray(wo[:, i])) for i in range(3)]
                t0, t1 = c.fresh(2)
                r.unop("MForm", a[0], t0)
                r.unop("MForm", a[1], t1)
                for x, y, z in ((t0, b[0], o2[0]), (t0, b[1], o2[1]), (t1, b[0], o2[1]), (t1, b[1], o2[2])):
                    r.binop("MulCoeffsMontgomeryThenAdd", x, y, z)
                assert np.array_equal(got, down(o2, level))
    a, _ = c.ct(2)
    b, _ = c.ct(2)
    out, _ = c.ct(3)
    assert _prof(ctx, lambda: K.ct_mul_relin_then_add(ks, c.top, a, b, None, out)) == {"tensor_add": 1}


@pytest.mark.parametrize("logN,nq,np_,B", [(12, 3, 2, 2), (12, 3, 1, 1), (10, 3, 2, 3)])
def test_mul_relin_then_add_with_a_key(ctx, logN, nq, np_, B):
    """(3 Q | 2 P) and a single special prime: the oracle's sequence, the composed sequence of today's entries, the census (the
    launches of he_relinearize at that shape plus one), every refused aliasing form"""
    from tests.conftest import Pi60, Qi60
    ks = KsCase(ctx, logN, Qi60[:nq], Pi60[:np_], 12600 + logN + np_)
    level = nq - 1
    for pre_on in (False, True):
        a, wa = ks.ct(2, B)
        b, wb = ks.ct(2, B)
        out, wo = ks.ct(2, B)
        pre = residues("uniform", ks.rng, ks.q) if pre_on else None
        K.ct_mul_relin_then_add(ks.gev, level, a, b, ks.grk, out, pre=pre)
        got = down(out, level)
        same(got, [REF.ckks_mul_relin_then_add(ks.oQ, level, list(wa[e]), list(wb[e]), list(wo[e]), pre, ks.oev, ks.ork) for e in range(B)], pre_on)
        assert np.array_equal(down(a, level), wa) and np.array_equal(down(b, level), wb)
        if not pre_on:  # composed: the three-component accumulation, then Relinearize of (0, 0, c2) onto the accumulator
            r = ks.gQ
            o2 = [la.Poly(ks.gQ, nq, B).upload(np.ascontiguousarray(wo[:, i])) for i in range(2)]
            t0, t1, c2 = (la.Poly(ks.gQ, nq, B) for _ in range(3))
            r.unop("MForm", a[0], t0)
            r.unop("MForm", a[1], t1)
            for x, y, z in ((t0, b[0], o2[0]), (t0, b[1], o2[1]), (t1, b[0], o2[1])):
                r.binop("MulCoeffsMontgomeryThenAdd", x, y, z)
            r.binop("MulCoeffsMontgomery", t1, b[1], c2)
            ks.gev.Relinearize(level, [o2[0], o2[1], c2], ks.grk, o2)
            assert np.array_equal(got, down(o2, level))
    # census
    a, _ = ks.ct(2, B)
    b, _ = ks.ct(2, B)
    out, _ = ks.ct(2, B)
    c2 = la.Poly(ks.gQ, nq, B)
    relin = _prof(ctx, lambda: ks.gev.Relinearize(level, [out[0], out[1], c2], ks.grk, out))
    mine = _prof(ctx, lambda: K.ct_mul_relin_then_add(ks.gev, level, a, b, ks.grk, out))
    assert mine.pop("tensor_add") == 1 and mine == relin, (mine, relin)
    # refusals: an output that is an input or the other output, out2 with a key; nothing changes
    assert A.ROWS["he_ckks_mul_relin_then_add"].allowed == set()
    everything = a + b + out
    before = [x.download().copy() for x in everything]
    for o in ([a[0], out[1]], [out[0], b[1]], [a[1], a[0]], [out[0], out[0]], [out[0], out[1], c2]):
        with pytest.raises(_lib.HeringError) as e:
            K.ct_mul_relin_then_add(ks.gev, level, a, b, ks.grk, o)
        assert e.value.code == -1
        ctx.sync()
        assert all(np.array_equal(x.download(), y) for x, y in zip(everything, before))
    with pytest.raises(_lib.HeringError):
        K.ct_mul_relin_then_add(ks.gev, level, a, b, None, out)  # no out2 without a key


# ---- census, poison, queue, graph, replay --------------------------------------------------------------------------------------------------
def test_launch_census_of_the_linear_entries(ctx):
    """each of the first three entries is exactly one launch of ct_lin_kernel, whatever the degrees and the form"""
    c = Case(ctx, 10, 3, 2, 12700)
    r = c.g
    p0, _ = c.ct(3)
    p1, _ = c.ct(2)
    (pt,), _ = c.ct(1, 1)
    out, _ = c.ct(3)
    s0, s1, pre = c.scal(2), c.scal(2), c.scal(2)
    for call in (lambda: K.ct_add(r, p0, p1, out, sub=True, scaled=2, ratio=pre), lambda: K.ct_add(r, p1, p0, out),
                 lambda: K.ct_scalar(r, 0, p0, s0, s1, out), lambda: K.ct_scalar(r, 1, p0, s0, s1, p0), lambda: K.ct_scalar(r, 2, p0, s0, s1, out),
                 lambda: K.ct_scalar(r, 3, p0, s0, s1, out, pre=pre), lambda: K.ct_mul_pt(r, p0, pt, out),
                 lambda: K.ct_mul_pt(r, p0, pt, out, then_add=True, pre=pre)):
        assert _prof(ctx, call) == {"ct_lin": 1}


def poison_case():
    """run by test_every_output_word_is_written in a process of its own with HERING_POISON=1: the outputs are scratch polynomials"""
    c0 = la.Context(0)
    for logN, nl, B in ((4, 3, 3), (10, 2, 1)):
        c = Case(c0, logN, nl, B, 12800 + logN, poison=True)
        level = c.top
        p0, w0 = c.ct(2)
        p1, w1 = c.ct(3)
        ratio, s0, s1 = c.scal(level), c.scal(level), c.scal(level)
        out = c.fresh(3)
        K.ct_add(c.g, p0, p1, out, sub=True, scaled=1, ratio=ratio)
        same(down(out, level), [REF.ckks_add(c.o, level, True, list(w0[b]), list(w1[b]), 1, ratio) for b in range(B)], "add")
        for op in (0, 2):
            out = c.fresh(3)
            K.ct_scalar(c.g, op, p1, s0, s1, out)
            same(down(out, level), [REF.ckks_scalar(c.o, level, op, list(w1[b]), s0, s1) for b in range(B)], op)
        out = c.fresh(3)
        K.ct_mul_pt(c.g, p1, p0[0], out)
        same(down(out, level), [REF.ckks_mul_pt(c.o, level, list(w1[b]), w0[b, 0]) for b in range(B)], "pt")
    c0.sync()


def test_every_output_word_is_written(ctx):
    env = dict(os.environ, HERING_POISON="1")
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_ckks_evaluator import poison_case; poison_case()"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("deferred", [0, 4])
def test_queue_coalesces_concurrent_callers(ctx, deferred):
    """four threads on their own batch-1 ciphertexts, each entry in turn: bit-identical to the direct calls, and fewer launches
    than calls (callers of one key ride in one launch over an entry table)"""
    c = Case(ctx, 10, 3, 1, 12900 + deferred)
    from tests.conftest import Pi60, Qi60
    ks = KsCase(ctx, 10, Qi60[:3], Pi60[:1], 12910 + deferred)
    TH, level, ROUNDS = 4, 2, 6
    ratio, s0, s1 = c.scal(level), c.scal(level), c.scal(level)
    data = []
    for t in range(TH):
        p0, w0 = c.ct(2)
        p1, w1 = c.ct(3)
        a, wa = ks.ct(2, 1)
        data.append((p0, w0, p1, w1, a, wa))
    (pt,), wp = c.ct(1)
    bb, _ = ks.ct(2, 1)

    def program(t, outs):
        p0, _, p1, _, a, _ = data[t]
        K.ct_add(c.g, p0, p1, outs[0], sub=True, scaled=2, ratio=ratio)
        K.ct_scalar(c.g, 3, p1, s0, s1, outs[0], pre=ratio)
        K.ct_mul_pt(c.g, p1, pt, outs[1])
        K.ct_mul_relin_then_add(ks.gev, level, a, bb, ks.grk, outs[2])

    def fresh_outs(t):
        return [c.fresh(3), c.fresh(3), [la.Poly(ks.gQ, 3, 1).upload(data[t][5][:, i].copy()) for i in range(2)]]

    want = []
    for t in range(TH):
        o = fresh_outs(t)
        program(t, o)
        want.append([down(x, level) for x in o])
    ctx.sync()
    outs = [fresh_outs(t) for t in range(TH)]
    ctx.SetCoalescing(64, 2000)
    if deferred:
        ctx.SetDeferred(deferred)
    try:
        st0 = ctx.CoalescingStats()
        barrier, errs = threading.Barrier(TH), []

        def worker(t):
            try:
                for k in range(ROUNDS):
                    barrier.wait()
                    o = fresh_outs(t) if k < ROUNDS - 1 else outs[t]
                    program(t, o)
            except Exception as e:  # noqa: BLE001
                errs.append(e)
                barrier.abort()

        th = [threading.Thread(target=worker, args=(t,)) for t in range(TH)]
        [x.start() for x in th]
        [x.join() for x in th]
        ctx.sync()
        assert not errs, errs
        st1 = ctx.CoalescingStats()
    finally:
        if deferred:
            ctx.SetDeferred(0)
        ctx.SetCoalescing(0, 0)
    for t in range(TH):
        for x, w in zip(outs[t], want[t]):
            assert np.array_equal(down(x, level), w), t
    calls, launches = st1["calls"] - st0["calls"], st1["launches"] - st0["launches"]
    assert calls >= TH * ROUNDS * 4 and launches < calls, (st0, st1)


def test_graph_capture_and_replay_program(ctx):
    """the four entries recorded under he_graph_begin / he_graph_end and launched; and recorded as a replay program (numbers 75 .. 78)
    run by two threads on their own polynomials"""
    c = Case(ctx, 10, 3, 1, 13000)
    from tests.conftest import Pi60, Qi60
    ks = KsCase(ctx, 10, Qi60[:3], Pi60[:1], 13010)
    level = 2
    ratio, s0, s1 = c.scal(level), c.scal(level), c.scal(level)
    p0, w0 = c.ct(2)
    p1, w1 = c.ct(3)
    (pt,), wp = c.ct(1)
    a, wa = ks.ct(2, 1)
    bb, _ = ks.ct(2, 1)
    acc, wacc = ks.ct(2, 1)

    def program(x0, o0, o1, o2):
        K.ct_add(c.g, x0, p1, o0, sub=True, scaled=2, ratio=ratio)
        K.ct_scalar(c.g, 3, p1, s0, s1, o0, pre=ratio)
        K.ct_mul_pt(c.g, p1, pt, o1)
        K.ct_mul_relin_then_add(ks.gev, level, a, bb, ks.grk, o2)

    def accs():
        return [la.Poly(ks.gQ, 3, 1).upload(wacc[:, i].copy()) for i in range(2)]

    o = [c.fresh(3), c.fresh(3), accs()]
    program(p0, *o)
    want = [down(x, level) for x in o]
    ctx.sync()
    g_out = [c.fresh(3), c.fresh(3), accs()]
    with ctx.capture() as g:
        program(p0, *g_out)
    g.launch()
    ctx.sync()
    for x, w in zip(g_out, want):
        assert np.array_equal(down(x, level), w)
    # the replay program: recorded once, run by two threads, each on its own input and outputs
    r_out = [c.fresh(3), c.fresh(3), accs()]
    ctx.sync()
    _lib.trace_begin()
    try:
        program(p0, *r_out)
    finally:
        prog = _lib.trace_end()
    fns, i = [], 0  # the program: [function, n args, args ...]; an argument is [kind, payload ...] (csrc/replay.cpp)
    while i < len(prog):
        fns.append(int(prog[i]))
        nargs, i = int(prog[i + 1]), i + 2
        for _ in range(nargs):
            kind = int(prog[i])
            i += {0: 2, 1: 2, 2: 2, 5: 1}[kind] if kind not in (3, 4) else 2 + int(prog[i + 1])
    assert fns == [75, 76, 77, 78]
    TH = 2
    mine = [[la.Poly(c.g, 3, 1).upload(w0[:, i].copy()) for i in range(2)] for _ in range(TH)]
    outs = [[c.fresh(3), c.fresh(3), accs()] for _ in range(TH)]
    flat = lambda x0, oo: [p.h for p in x0] + [p.h for grp in oo for p in grp]
    sf = flat(p0, r_out)
    st = [flat(mine[t], outs[t]) for t in range(TH)]
    ctx.sync()
    _lib.replay(ctx.h, prog, TH, 1, sf, st, [])
    ctx.sync()
    for t in range(TH):
        for x, w in zip(outs[t], want):
            assert np.array_equal(down(x, level), w), t


# ---- the mirror: lattigo_amd.ckks.Evaluator over rlwe.Ciphertext / Plaintext with metadata ------------------------------------------------
def test_mirror_program_against_the_oracle_evaluator(ctx):
    """a short program through ckks.Evaluator -- ciphertext, plaintext and scalar operands, differing scales (both directions of
    the scale matching), Mul / MulRelin / MulThenAdd / MulRelinThenAdd with the scale-up of the accumulator, Relinearize, Rescale
    -- every result's words, level, degree and Scale against oracle/circuits.CKKSCtEvaluator (exact rational scales, which the
    128-bit scales equal until the Rescale) and tests/ckks_evaluator_ref.py (its Scale after the Rescale, bit for bit)"""
    from fractions import Fraction
    from lattigo_amd import rlwe as RL
    from oracle import circuits as OC
    from tests.conftest import Pi60, Qi60
    ks = KsCase(ctx, 10, Qi60[:3], Pi60[:2], 13100)
    S0 = 1 << 45
    params = K.Parameters(ks.gQ, S0)
    ev = K.Evaluator(params, ks.gev, ks.grk)
    oe = OC.CKKSCtEvaluator(ks.oev, ks.ork, float(S0))
    top = 2

    def pair(n, scale):
        polys, w = ks.ct(n, 1)
        g = (RL.Ciphertext(ks.gQ, n - 1, top, 1, Value=polys, MetaData_=RL.MetaData(scale)) if n > 1
             else RL.Plaintext(ks.gQ, top, 1, Value=polys, MetaData_=RL.MetaData(scale)))
        return g, OC.Ct(list(w[0]), Fraction(scale))

    def check(g, o, tag):
        assert (g.Level(), g.Degree()) == (o.level, o.Degree()), tag
        assert g.Scale.Value == Fraction(o.Scale), tag
        assert np.array_equal(down(g.Value, g.Level())[0], np.stack([v[: o.level + 1] for v in o.Value])), tag

    ga, oa = pair(2, S0)
    gb, ob = pair(2, 3 * S0)
    gp, op = pair(1, S0)
    for name, x, y in (("Add", (ga, gb), (oa, ob)), ("Add", (gb, ga), (ob, oa)), ("Sub", (ga, gb), (oa, ob)), ("Sub", (gb, ga), (ob, oa)),
                       ("Add", (ga, gp), (oa, op)), ("Sub", (gb, gp), (ob, op)), ("Add", (ga, ga), (oa, oa))):
        g = getattr(ev, name + "New")(*x)
        o = oe.NewCiphertext(1, top)
        getattr(oe, name)(*y, o)
        check(g, o, (name, "ct"))
        assert g.Scale.Value == max(x[0].Scale.Value, x[1].Scale.Value)
    for c in (0.5, 3, -2.25 + 1.5j, Fraction(1, 3)):
        for name in ("Add", "Sub", "Mul"):
            g = getattr(ev, name + "New")(ga, c)
            o = oe.NewCiphertext(1, top)
            getattr(oe, name)(oa, c, o)
            check(g, o, (name, c))
    g = ev.MulNew(ga, gp)
    o = oe.NewCiphertext(1, top)
    oe.Mul(oa, op, o)
    check(g, o, "Mul pt")
    g2 = ev.MulNew(ga, gb)
    o2 = oe.NewCiphertext(2, top)
    oe.Mul(oa, ob, o2)
    check(g2, o2, "Mul ct")
    gr = ev.RelinearizeNew(g2)
    orl = oe.NewCiphertext(1, top)
    oe.Relinearize(o2, orl)
    check(gr, orl, "Relinearize")
    gm = ev.MulRelinNew(ga, gb)
    om = oe.NewCiphertext(1, top)
    oe.MulRelin(oa, ob, om)
    check(gm, om, "MulRelin")
    # MulThenAdd with a scalar: equal scales and a non-integer (the accumulator is multiplied by q_level first), an integer, and an
    # accumulator of a larger scale
    for c, acc_scale in ((0.25, S0), (7, S0), (0.25, 3 * S0)):
        gacc, oacc = pair(2, acc_scale)
        ev.MulThenAdd(ga, c, gacc)
        oe.MulThenAdd(oa, c, oacc)
        check(gacc, oacc, ("MulThenAdd", c, acc_scale))
    # MulRelinThenAdd / MulThenAdd onto an accumulator of the scale of one operand: ratio = 3 * 2^45, an integer
    ratio = np.array([(3 * S0) % int(q) for q in ks.q], dtype=np.uint64)
    for relin in (True, False):
        gacc, oacc = pair(2, S0)
        (ev.MulRelinThenAdd if relin else ev.MulThenAdd)(ga, gb, gacc)
        acc = oacc.Value + ([np.zeros_like(oacc.Value[0])] if not relin else [])
        want = REF.ckks_mul_relin_then_add(ks.oQ, top, oa.Value, ob.Value, acc, ratio, ks.oev if relin else None, ks.ork if relin else None)
        assert gacc.Degree() == (1 if relin else 2) and gacc.Scale.Value == Fraction(3 * S0 * S0)
        assert np.array_equal(down(gacc.Value, top)[0], np.stack(want)), relin
    gacc, oacc = pair(2, S0)
    ev.MulThenAdd(gb, gp, gacc)
    want = REF.ckks_mul_pt(ks.oQ, top, ob.Value, op.Value[0], oacc.Value, ratio)
    assert np.array_equal(down(gacc.Value, top)[0], np.stack(want)) and gacc.Scale.Value == Fraction(3 * S0 * S0)
    with pytest.raises(ValueError, match="opOut must be different from op0 and op1"):
        ev.MulRelinThenAdd(ga, gb, ga)
    with pytest.raises(ValueError, match="op0.Scale > opOut.Scale is not supported"):
        ev.MulThenAdd(gb, 0.5, pair(2, S0)[0])
    # Rescale: the scale is now a rounded 128-bit float
    ev.Rescale(gm, gm)
    ors = oe.NewCiphertext(1, top - 1)
    oe.Rescale(om, ors)
    assert (gm.Level(), gm.Degree()) == (top - 1, 1)
    assert np.array_equal(down(gm.Value, top - 1)[0], np.stack(ors.Value))
    assert gm.Scale.Value == REF.Scale(3 * S0 * S0).Div(int(ks.q[top])).fraction() != Fraction(ors.Scale)
    g = ev.DropLevelNew(ga, 1)
    assert g.Level() == top - 1 and ga.Level() == top and np.array_equal(down(g.Value, top - 1), down(ga.Value, top - 1))


def test_mirror_nine_scale_matching_branches(ctx):
    """evaluateInPlace: opOut is op0, is op1 or is neither, times op0's scale greater, smaller or equal -- the scale-aligned sum
    (the oracle evaluator's, on the pre-call words) and the larger scale, with op1 of a higher degree so that the tail is scaled too"""
    from fractions import Fraction
    from lattigo_amd import rlwe as RL
    from oracle import circuits as OC
    from tests.conftest import Pi60, Qi60
    ks = KsCase(ctx, 10, Qi60[:2], Pi60[:1], 13200)
    S0 = 1 << 40
    ev = K.Evaluator(K.Parameters(ks.gQ, S0), ks.gev, None)
    oe = OC.CKKSCtEvaluator(ks.oev, None, float(S0))
    for sub in (False, True):
        for s0, s1 in ((5 * S0, S0), (S0, 5 * S0), (S0, S0), (S0 * 7, S0 * 2)):  # (the last: a truncated ratio, 3)
            for target in ("op0", "op1", "new"):
                n0, n1 = (3, 3) if target != "new" else (2, 3)
                p0, w0 = ks.ct(n0, 1)
                p1, w1 = ks.ct(n1, 1)
                g0 = RL.Ciphertext(ks.gQ, n0 - 1, 1, 1, Value=p0, MetaData_=RL.MetaData(s0))
                g1 = RL.Ciphertext(ks.gQ, n1 - 1, 1, 1, Value=p1, MetaData_=RL.MetaData(s1))
                o = oe.NewCiphertext(2, 1)
                (oe.Sub if sub else oe.Add)(OC.Ct(list(w0[0]), Fraction(s0)), OC.Ct(list(w1[0]), Fraction(s1)), o)
                out = {"op0": g0, "op1": g1, "new": K.NewCiphertext(ev.params, 2, 1)}[target]
                (ev.Sub if sub else ev.Add)(g0, g1, out)
                assert out.Scale.Value == max(s0, s1) == Fraction(o.Scale) and out.Degree() == 2, (sub, s0, s1, target)
                assert np.array_equal(down(out.Value, 1)[0], np.stack(o.Value)), (sub, s0, s1, target)


def test_mirror_scale_up_rescale_new_and_with_key(ctx):
    from fractions import Fraction
    from lattigo_amd import rlwe as RL
    from oracle import circuits as OC
    from tests.conftest import Pi60, Qi60
    ks = KsCase(ctx, 10, Qi60[:3], Pi60[:1], 13400)
    S0 = 1 << 45
    ev = K.Evaluator(K.Parameters(ks.gQ, S0), ks.gev, ks.grk)
    oe = OC.CKKSCtEvaluator(ks.oev, ks.ork, float(S0))
    polys, w = ks.ct(2, 1)
    g = RL.Ciphertext(ks.gQ, 1, 2, 1, Value=polys, MetaData_=RL.MetaData(S0))
    o = OC.Ct(list(w[0]), Fraction(S0))
    up = ev.ScaleUpNew(g, RL.Scale(4.75))  # :433-443: multiplied by Uint64(4.75) = 4, the scale by 4.75
    want = oe.NewCiphertext(1, 2)
    oe.Mul(o, 4, want)
    assert up.Scale.Value == Fraction(S0) * Fraction(4.75) and np.array_equal(down(up.Value, 2)[0], np.stack(want.Value))
    rs = ev.RescaleNew(g)
    want = oe.NewCiphertext(1, 1)
    oe.Rescale(o, want)
    assert rs.Level() == 1 and g.Level() == 2 and np.array_equal(down(rs.Value, 1)[0], np.stack(want.Value))
    assert rs.Scale.Value == REF.Scale(S0).Div(int(ks.q[2])).fraction()
    nokey = ev.WithKey(None)
    with pytest.raises(ValueError, match="EvaluationKeySet is nil"):
        nokey.MulRelinNew(g, g)
    with pytest.raises(ValueError, match="EvaluationKeySet is nil"):
        nokey.MulRelinThenAdd(g, g, ev.MulRelinNew(g, g))
    with pytest.raises(ValueError, match="already at level 0"):
        ev.Rescale(ev.DropLevelNew(g, 2), K.NewCiphertext(ev.params, 1, 0))
    with pytest.raises(ValueError, match="above 2\\^60"):
        K.Parameters(ks.gQ, 1 << 80)
    cp = g.CopyNew()
    assert cp.Scale.Value == g.Scale.Value and np.array_equal(down(cp.Value, 2), down(g.Value, 2)) and cp.Value[0].h != g.Value[0].h


# ---- all q - 1 and all zero on every operand of every form ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["max", "zero"])
def test_every_operand_all_max_or_all_zero(ctx, kind):
    """every word of every operand q - 1 (the worst-case sums: (q - 1) + (q - 1), r (q - 1) + (q - 1)^2, and in the tensor
    acc + (m1 + m2) at the 61-bit prime) or 0, scalar / ratio / pre words q - 1 as well: every form of the four entries, with and
    without a key, against the restatement and plain arithmetic"""
    from tests.conftest import Pi60, Qi60
    c = Case(ctx, 4, 3, 2, 13600)
    level, B = 2, 2

    def ct(n, ring=None, q=None):
        q = c.q if q is None else q
        w = np.stack([np.stack([words(kind, c.rng, q, c.N) for _ in range(n)]) for _ in range(B)])
        return [la.Poly(ring or c.g, len(q), B).upload(np.ascontiguousarray(w[:, i])) for i in range(n)], w

    top = np.array([m - 1 for m in c.q], dtype=np.uint64)
    for n0, n1 in ((2, 2), (1, 3), (3, 2)):
        for sub in (False, True):
            for scaled in (0, 1, 2):
                p0, w0 = ct(n0)
                p1, w1 = ct(n1)
                out = c.fresh(max(n0, n1))
                K.ct_add(c.g, p0, p1, out, sub=sub, scaled=scaled, ratio=top if scaled else None)
                got = down(out, level)
                same(got, [REF.ckks_add(c.o, level, sub, list(w0[b]), list(w1[b]), scaled, top) for b in range(B)], (n0, n1, sub, scaled))
                same(got, [REF.exact_add(c.o, level, sub, list(w0[b]), list(w1[b]), scaled, top) for b in range(B)], (n0, n1, sub, scaled))
    for op in range(4):
        for pre in ((None, top) if op == 3 else (None,)):
            p0, w0 = ct(3)
            out, wo = ct(3)
            K.ct_scalar(c.g, op, p0, top, top, out, pre=pre)
            got = down(out, level)
            same(got, [REF.ckks_scalar(c.o, level, op, list(w0[b]), top, top, list(wo[b]), pre) for b in range(B)], (op, pre is not None))
            same(got, [REF.exact_scalar(c.o, level, op, list(w0[b]), top, top, list(wo[b]), pre) for b in range(B)], (op, pre is not None))
    for then_add, pre in ((False, None), (True, None), (True, top)):
        p0, w0 = ct(3)
        (pt,), wp = ct(1)
        out, wo = ct(3)
        K.ct_mul_pt(c.g, p0, pt, out, then_add=then_add, pre=pre)
        got = down(out, level)
        args = lambda b: (c.o, level, list(w0[b]), wp[b, 0], list(wo[b]) if then_add else None, pre)
        same(got, [REF.ckks_mul_pt(*args(b)) for b in range(B)], (then_add, pre is not None))
        same(got, [REF.exact_mul_pt(*args(b)) for b in range(B)], (then_add, pre is not None))
    nokey = la.Evaluator(c.g, None)
    for pre in (None, top):
        a, wa = ct(2)
        b_, wb = ct(2)
        out, wo = ct(3)
        K.ct_mul_relin_then_add(nokey, level, a, b_, None, out, pre=pre)
        got = down(out, level)
        same(got, [REF.ckks_mul_relin_then_add(c.o, level, list(wa[e]), list(wb[e]), list(wo[e]), pre) for e in range(B)], pre is not None)
        same(got, [REF.exact_mul_then_add(c.o, level, list(wa[e]), list(wb[e]), list(wo[e]), pre) for e in range(B)], pre is not None)
    for logN, np_ in ((12, 2), (10, 1)):
        ks = KsCase(ctx, logN, Qi60[:3], Pi60[:np_], 13610 + logN)
        ktop = np.array([m - 1 for m in ks.q], dtype=np.uint64)
        c.N = ks.N
        for pre in (None, ktop):
            a, wa = ct(2, ks.gQ, ks.q)
            b_, wb = ct(2, ks.gQ, ks.q)
            out, wo = ct(2, ks.gQ, ks.q)
            K.ct_mul_relin_then_add(ks.gev, 2, a, b_, ks.grk, out, pre=pre)
            same(down(out, 2), [REF.ckks_mul_relin_then_add(ks.oQ, 2, list(wa[e]), list(wb[e]), list(wo[e]), pre, ks.oev, ks.ork) for e in range(B)],
                 (logN, pre is not None))
    c.N = 16


# ---- encode -> encrypt -> evaluate -> decrypt -> decode with generated keys ------------------------------------------------------------------
def test_mirror_end_to_end_with_generated_keys(ctx):
    """Keys from rlwe.KeyGenerator on the device, ckks.Encoder, Encryptor under pk; a program through ckks.Evaluator with scalar,
    vector, plaintext and ciphertext operands, differing scales, MulRelinThenAdd, Rescale, SetScale, ScaleUp, DropLevel, Rotate,
    Conjugate, RotateHoisted, InnerSum, RotateAndAdd and ApplyEvaluationKey; Decryptor and Decode.

    First leg: the generated keys and the fresh ciphertexts' words are downloaded, and tests/ckks_evaluator_ref.RefEvaluator (the
    reference line by line on the oracle) runs the same program on them; a vector operand reaches it through the same encoder.
    After every step the words, the level, the degree and the Scale (bit for bit) are equal.

    Second leg: every intermediate decrypts to the same computation in complex128.  Bound: logN 10, scale S = 2^45, values in the
    unit box.  A fresh encryption under pk has noise u e_pk + e0 + e1 s with ternary u, s and |e| <= 19: below 19 (2 N + 1) < 2^16
    per coefficient; a key switch adds less than that after its division by P (tests/test_gpu_keygen.py derives both), a rescale
    adds (1 + N) / 2 < 2^10, an encoding rounds by 1/2 per coefficient.  A product multiplies the noise of one factor by the
    other's message, at most S N in a coefficient, and the rescale divides by q ~ S again.  So every result carries coefficient
    noise below 2^16 N 8 < 2^30 at a scale of at least S / 4 = 2^43, and a slot, a sum of N coefficients times roots of modulus 1,
    is off by less than 2^30 N / 2^43 = 2^-3 in the very worst case; the standard deviation is about sqrt(N) times smaller per sum
    and 19 / 3.2 times smaller per term, 2^-3 / (32 * 32 * 6) ~ 2^-16, and six of those stay below 2^-13.  (A worst-case bound: what
    is seen is around 2^-34; the words are what the first leg pins.)"""
    from lattigo_amd import encryptor as E
    from lattigo_amd import keygen as G
    from lattigo_amd import rlwe as RL
    from lattigo_amd import sampling
    from tests import sampler_ref as SR
    logN = 10
    N, nth, slots = 1 << logN, 2 << logN, 1 << (logN - 1)
    q, p = O.GenModuli(logN + 1, [55] + [45] * 5, [55, 55])
    gQ, gP = la.Ring(ctx, N, q), la.Ring(ctx, N, p)
    rev = la.Evaluator(gQ, gP)
    prng = sampling.PRNG(SR.seeded_source(13700).read)
    kg = G.KeyGenerator(rev, prng)
    sk, pk = kg.GenKeyPairNew()
    rlk = kg.GenRelinearizationKeyNew(sk)
    galels = sorted({RL.GaloisElement(nth, 1), RL.GaloisElement(nth, 3), nth - 1} | set(RL.GaloisElementsForInnerSum(nth, 1, 4))
                    | set(RL.GaloisElementsForInnerSum(nth, 2, 3)))
    gks = RL.GaloisKeySet({gk.GaloisElement: gk.EvaluationKey for gk in kg.GenGaloisKeysNew(galels, sk)})
    swk = kg.GenEvaluationKeyNew(sk, sk)
    encoder = K.Encoder(gQ, gP)
    S = 1 << 45
    params = K.Parameters(gQ, S, gP)
    ev = K.Evaluator(params, rev, rlk, gks, encoder)
    top = len(q) - 1
    rng = rng_for(13701)
    vec = lambda: rng.uniform(-1, 1, slots) + 1j * rng.uniform(-1, 1, slots)
    encryptor, decryptor = E.Encryptor(rev, prng, pk), E.Decryptor(rev, sk)
    # the restatement on the oracle, on the downloaded keys
    okey = lambda k: (lambda w: O.EvaluationKey(np.ascontiguousarray(w[:, :, : len(q)]), np.ascontiguousarray(w[:, :, len(q):])))(k.download())
    hook = lambda values, level, scale: encoder.Encode(values, la.Poly(gQ, level + 1, 1), Scale=scale, level=level).download()[0]
    rf = REF.RefEvaluator(O.Evaluator(O.Ring(N, q), O.Ring(N, p)), S, okey(rlk), {g: okey(k) for g, k in gks.keys.items()}, hook)

    def mirror_of(g):
        return REF.RefCt([v.download()[0][: g.Level() + 1] for v in g.Value], g.Scale.Value, 9)

    def plaintext(v, scale):
        return K.FromPolys(params, [encoder.Encode(v, gQ.NewPoly(), Scale=float(scale))], top, scale)

    def encrypt(v, scale):
        ct = E.Element([gQ.NewPoly(), gQ.NewPoly()])
        encryptor.Encrypt(E.Plaintext(plaintext(v, scale).Value[0]), ct)
        return K.FromPolys(params, ct.Value, top, scale)

    worst = [0.0]

    def check(ct, o, want, tag):
        # first leg: the restatement's words and metadata
        assert (ct.Level(), ct.Degree()) == (o.Level(), o.Degree()), tag
        assert ct.Scale.Value == o.Scale.fraction(), tag
        assert np.array_equal(down(ct.Value, ct.Level())[0], np.stack([v[: o.Level() + 1] for v in o.Value])), tag
        # second leg: decryption
        level = ct.Level()
        pt = E.Plaintext(la.Poly(gQ, level + 1, 1))
        cut = []
        for v in ct.Value:  # (a component may be taller than the element's level)
            w = la.Poly(gQ, level + 1, 1)
            w.CopyLvl(level, v)
            cut.append(w)
        decryptor.Decrypt(E.Element(cut, True, False), pt)
        got = encoder.Decode(pt.Value, Scale=ct.Scale.Float64(), level=level)[0]
        err = float(np.max(np.abs(got - want)))
        worst[0] = max(worst[0], err)
        print(tag, "level", level, "log2 scale", round(float(np.log2(ct.Scale.Float64())), 3), "error 2^", round(float(np.log2(err + 1e-300)), 1))
        assert err < 2.0 ** -13, (tag, err)

    def both(name, gargs, oargs, want, tag, out=None):
        """the method `name` of the mirror and of the restatement, into new outputs of the shape `out` = (degree, level)"""
        degree, level = out if out is not None else (1, top)
        g, o = K.NewCiphertext(params, degree, level), rf.NewCiphertext(degree, level)
        getattr(ev, name)(*gargs, g)
        getattr(rf, name)(*oargs, o)
        check(g, o, want, tag)
        return g, o

    x, y, z, w, v = vec(), vec(), vec(), vec(), vec()
    a, b, a2, ptw = encrypt(x, S), encrypt(y, 3 * S), encrypt(z, S), plaintext(w, S)
    oa, ob, oa2, optw = mirror_of(a), mirror_of(b), mirror_of(a2), mirror_of(ptw)
    check(a, oa, x, "fresh")
    c, oc = both("Add", (a, b), (oa, ob), x + y, "Add of different scales")
    assert c.Scale.Value == 3 * S
    both("Sub", (b, a), (ob, oa), y - x, "Sub of different scales")
    both("Add", (a, ptw), (oa, optw), x + w, "Add plaintext")
    both("Add", (a, 0.5 - 2j), (oa, 0.5 - 2j), x + 0.5 - 2j, "Add scalar")
    both("Sub", (a, 3), (oa, 3), x - 3, "Sub integer")
    both("Sub", (a, v), (oa, v), x - v, "Sub vector")
    d, od = both("Mul", (c, 0.5), (oc, 0.5), 0.5 * (x + y), "Mul scalar")
    assert d.Scale.Value == RL.Scale(3 * S).Mul(q[top]).Value
    ev.Rescale(d, d)
    rf.Rescale(od, od)
    check(d, od, 0.5 * (x + y), "Rescale")
    e, oe_ = both("Add", (d, v), (od, v), 0.5 * (x + y) + v, "Add vector", (1, top - 1))
    m, om = both("Mul", (a, v), (oa, v), x * v, "Mul vector")
    both("Rescale", (m,), (om,), x * v, "Rescale of Mul vector")
    f, of = both("MulRelin", (e, a), (oe_, oa), (0.5 * (x + y) + v) * x, "MulRelin", (1, top - 1))
    ev.Rescale(f, f)
    rf.Rescale(of, of)
    fw = (0.5 * (x + y) + v) * x
    check(f, of, fw, "MulRelin, Rescale")
    assert f.Scale.Value.denominator != 1  # a quotient by an odd prime: rounded 128-bit scales from here on
    acc, oacc = both("Mul", (a, ptw), (oa, optw), x * w, "Mul plaintext")
    ev.MulRelinThenAdd(a, a2, acc)
    rf.MulRelinThenAdd(oa, oa2, oacc)
    check(acc, oacc, x * w + x * z, "MulRelinThenAdd")
    acc3, oacc3 = both("Mul", (a, a2), (oa, oa2), x * z, "Mul ciphertext", (2, top))
    ev.MulThenAdd(a2, a, acc3)
    rf.MulThenAdd(oa2, oa, oacc3)
    check(acc3, oacc3, 2 * x * z, "MulThenAdd degree 2")
    both("Relinearize", (acc3,), (oacc3,), 2 * x * z, "Relinearize")
    low, olow = a.CopyNew(), oa.CopyNew()
    ev.MulRelinThenAdd(b, a2, low)  # the accumulator is scaled up by 3 S first
    rf.MulRelinThenAdd(ob, oa2, olow)
    assert low.Scale.Value == 3 * S * S
    check(low, olow, x + y * z, "MulRelinThenAdd with a scale-up")
    for const, want, tag in ((0.25, x + 0.25 * z, "MulThenAdd scalar"), (v, x + z * v, "MulThenAdd vector"), (ptw, None, None)):
        g, o = a.CopyNew(), oa.CopyNew()
        if tag is None:
            g, o = ev.MulNew(a, ptw), rf.NewCiphertext(1, top)
            rf.Mul(oa, optw, o)
            ev.MulThenAdd(a2, ptw, g)
            rf.MulThenAdd(oa2, optw, o)
            check(g, o, x * w + z * w, "MulThenAdd plaintext")
            continue
        ev.MulThenAdd(a2, const, g)  # equal scales: the accumulator is multiplied by q_top
        rf.MulThenAdd(oa2, const, o)
        check(g, o, want, tag)
    both("MulRelin", (a, 0.5), (oa, 0.5), 0.5 * x, "MulRelin with a scalar is Mul")
    g, o = a.CopyNew(), oa.CopyNew()
    ev.MulRelinThenAdd(a2, 2, g)
    rf.MulRelinThenAdd(oa2, 2, o)
    check(g, o, x + 2 * z, "MulRelinThenAdd with a scalar is MulThenAdd")
    both("ScaleUp", (a, RL.Scale(4.75)), (oa, REF.Scale(4.75)), x * 4 / 4.75, "ScaleUp")
    dl, odl = ev.DropLevelNew(a, 2), oa.CopyNew()
    rf.DropLevel(odl, 2)
    check(dl, odl, x, "DropLevel")
    ev.SetScale(f, S)
    rf.SetScale(of, S)
    assert f.Scale.Value == S and f.Level() == top - 3
    check(f, of, fw, "SetScale")
    lv = f.Level()
    both("Rotate", (f, 1), (of, 1), np.roll(fw, -1), "Rotate", (1, lv))
    both("Conjugate", (f,), (of,), np.conj(fw), "Conjugate", (1, lv))
    hg = ev.RotateHoistedNew(f, [1, 3])
    ho = {k: rf.NewCiphertext(1, lv) for k in (1, 3)}
    rf.RotateHoisted(of, [1, 3], ho)
    for k in (1, 3):
        check(hg[k], ho[k], np.roll(fw, -k), f"RotateHoisted {k}")
    both("InnerSum", (f, 1, 4), (of, 1, 4), sum(np.roll(fw, -i) for i in range(4)), "InnerSum", (1, lv))
    both("RotateAndAdd", (f, 2, 3), (of, 2, 3), sum(np.roll(fw, -2 * i) for i in range(3)), "RotateAndAdd", (1, lv))
    both("ApplyEvaluationKey", (f, swk), (of, okey(swk)), fw, "ApplyEvaluationKey", (1, lv))
    both("RescaleTo", (acc, RL.Scale(S)), (oacc, REF.Scale(S)), x * w + x * z, "RescaleTo")
    dec = RL.Decomposition(rev, 1)
    rev.DecomposeNTT(lv, gP.MaxLevel(), gP.MaxLevel() + 1, f.Value[1], True, dec)
    lazy = ev.RotateHoistedLazyNew(lv, [0, 3], f, dec)
    assert sorted(lazy) == [3]
    with pytest.raises(ValueError, match="but is str"):
        ev.Add(a, "x", a)
    with pytest.raises(ValueError, match="but is dict"):
        ev.MulThenAdd(a, {}, acc)
    with pytest.raises(ValueError, match="cannot Rotate: .*GaloisKey\\[.*\\] is nil"):
        ev.RotateNew(f, 7)
    assert worst[0] < 2.0 ** -13


def test_mirror_equals_the_restatement_word_for_word(ctx):
    """the same program through lattigo_amd.ckks.Evaluator and through tests/ckks_evaluator_ref.RefEvaluator (the reference line by
    line on the oracle, with a Scale of its own) on the same words and keys: after every step the words, the level, the degree and
    the Scale bit for bit -- through Rescale, SetScale and RescaleTo, where the scales are rounded 128-bit floats"""
    from fractions import Fraction
    from lattigo_amd import rlwe as RL
    from tests.conftest import Pi60, Qi60
    ks = KsCase(ctx, 10, Qi60[:4], Pi60[:2], 13900)
    top, S0, N = 3, 1 << 45, ks.N
    g1 = RL.GaloisElement(2 * N, 1)
    beta = O.BaseRNSDecompositionVectorSize(top, 1)
    kq = np.stack([np.stack([uniform_poly(ks.rng, ks.q, N) for _ in range(2)]) for _ in range(beta)])
    kp = np.stack([np.stack([uniform_poly(ks.rng, ks.p, N) for _ in range(2)]) for _ in range(beta)])
    ogk, ggk = O.EvaluationKey(kq, kp), ks.gev.NewEvaluationKey(kq, kp)
    params = K.Parameters(ks.gQ, S0, ks.gP)
    ev = K.Evaluator(params, ks.gev, ks.grk, RL.GaloisKeySet({g1: ggk}))
    rf = REF.RefEvaluator(ks.oev, S0, ks.ork, {g1: ogk})

    def pair(n, scale):
        polys, w = ks.ct(n, 1)
        g = K.FromPolys(params, polys, top, scale)
        return g, REF.RefCt(list(w[0]), scale, 9)

    step = [0]

    def check(g, o):
        step[0] += 1
        assert (g.Level(), g.Degree()) == (o.Level(), o.Degree()), step
        assert g.Scale.Value == o.Scale.fraction(), step
        assert np.array_equal(down(g.Value, g.Level())[0], np.stack([v[: o.Level() + 1] for v in o.Value])), step

    ga, oa = pair(2, S0)
    gb, ob = pair(2, Fraction(7 * S0, 2))  # a truncated ratio, 3
    gp, op = pair(1, S0)
    gc, oc = ev.AddNew(ga, gb), rf.NewCiphertext(1, top)
    rf.Add(oa, ob, oc)
    check(gc, oc)
    ev.Sub(gc, ga, gc)  # opOut is op0, the other operand is scaled
    rf.Sub(oc, oa, oc)
    check(gc, oc)
    gd, od = ev.MulNew(gc, 0.37 - 0.2j), rf.NewCiphertext(1, top)
    rf.Mul(oc, 0.37 - 0.2j, od)
    check(gd, od)
    ev.Rescale(gd, gd)
    rf.Rescale(od, od)
    check(gd, od)
    ge, oe_ = ev.MulRelinNew(gd, ga), rf.NewCiphertext(1, top - 1)
    rf.MulRelin(od, oa, oe_)
    check(ge, oe_)
    ev.Rescale(ge, ge)
    rf.Rescale(oe_, oe_)
    check(ge, oe_)
    assert ge.Scale.Value.denominator != 1  # a quotient by an odd prime: a rounded 128-bit float from here on
    ev.Add(ge, gd, ge)  # a rounded scale against an exact one: a large truncated ratio
    rf.Add(oe_, od, oe_)
    check(ge, oe_)
    gacc, oacc = pair(2, S0)
    ev.MulRelinThenAdd(gd, ga, gacc)  # the scale-up by a non-integer ratio, encoded at q_level as the reference does
    rf.MulRelinThenAdd(od, oa, oacc)
    check(gacc, oacc)
    gacc, oacc = pair(2, Fraction(7 * S0, 2))  # gd's scale: equal scales and a non-integer constant
    ev.MulThenAdd(gd, 0.25, gacc)  # op0 one level below the accumulator: the scale-up runs over all of the accumulator's limbs
    rf.MulThenAdd(od, 0.25, oacc)
    assert gacc.Level() == top
    check(gacc, oacc)
    gacc, oacc = pair(2, S0)
    ev.MulThenAdd(ga, gp, gacc)
    rf.MulThenAdd(oa, op, oacc)
    check(gacc, oacc)
    ev.SetScale(ge, S0)
    rf.SetScale(oe_, S0)
    check(ge, oe_)
    gr, orr = ev.RotateNew(ge, 1), rf.NewCiphertext(1, ge.Level())
    rf.Rotate(oe_, 1, orr)
    check(gr, orr)
    gt, ot = K.NewCiphertext(params, 1, top), rf.NewCiphertext(1, top)
    ev.RescaleTo(gacc, Fraction(S0, 3), gt)
    rf.RescaleTo(oacc, Fraction(S0, 3), ot)
    check(gt, ot)
