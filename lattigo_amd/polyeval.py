"""circuits/common/polynomial on the device (include/hering_polyeval.h), with its two instantiations circuits/bgv/polynomial and
circuits/ckks/polynomial.  The structure of an evaluation -- which powers are made and how, the Paterson-Stockmeyer decomposition,
the order of the giant steps -- is the library's (``Plan``, csrc/polyeval_plan.h through he_polyeval_plan).  This module
plans what the library leaves to its callers: the scales (exact rationals for CKKS, residues mod t for BGV, as the ``Scheme``
objects carry them) and the scalar words of every baby step.  ``Polynomial.Plan`` turns a polynomial, an input (level, scale)
and a target scale into a ``PlannedPolynomial``: the native handle with the words uploaded once, whose
``EvaluatePolynomialFromPowerBasis`` runs a run of baby steps as one fused launch per group.  ``Evaluator`` is
polynomial.Evaluator: ``Evaluate``, ``EvaluateFromPowerBasis`` and ``GenPower`` are one native call each over a device
``PowerBasis``; what this module adds to them is the planning."""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction

import numpy as np

from lattigo_amd._lib import H, check, load, u64p

MAX_TERMS = 31
_OPS = ("CopyNew", "Relinearize", "Rescale", "MulNew", "MulRelinNew", "Add", "Add", "Sub", "NewCiphertext", "Add", "MulThenAdd", "Mul", "Add")
OP_COPY, OP_RELIN, OP_RESCALE, OP_MUL_NEW, OP_MUL_RELIN_NEW, OP_ADD_SELF, OP_ADD_MINUS_ONE, OP_SUB, OP_NEW, OP_ADD_CONST, \
    OP_MUL_THEN_ADD, OP_MUL, OP_ADD = range(13)


def _ints(v):
    v = [int(x) for x in v]
    return (C.c_int * max(len(v), 1))(*v), len(v)


def OptimalSplit(logDegree: int) -> int:
    """utils/bignum/polynomial.go:14"""
    out = C.c_int()
    check(load().he_polyeval_optimal_split(int(logDegree), C.byref(out)))
    return out.value


def SplitDegree(n: int):
    """circuits/common/polynomial/power_basis.go:31"""
    a, b = C.c_int(), C.c_int()
    check(load().he_polyeval_split_degree(int(n), C.byref(a), C.byref(b)))
    return a.value, b.value


def Depth(degree: int, level: int | None = None) -> int:
    """ceil(log2 degree); with a level, the depth check of Evaluate (polynomial_evaluator.go:62-65): raises below it"""
    out = C.c_int()
    check(load().he_polyeval_depth(int(degree), (1 << 30) if level is None else int(level), C.byref(out)))
    return out.value


class Plan:
    """the library's structure of one evaluation: ``leaves`` = [(degree, level, new_degree, ct_degree, present)], ``steps`` =
    [(op, dst, level, degree, a, b)] in the order of the reference's primitive calls (a power is n >= 1, baby step i is -1 - i)"""

    def __init__(self, degree, basis="Monomial", even=True, odd=True, lazy=False, powers=None, level=None, copy_input=True):
        powers = {1: (int(level), 1)} if powers is None else powers
        flat, n = _ints([v for k in sorted(powers) for v in (k, powers[k][0], powers[k][1])])
        args = (int(degree), 1 if basis == "Chebyshev" else 0, int(bool(even)), int(bool(odd)), int(bool(lazy)), int(bool(copy_input)), n // 3, flat)
        got = C.c_size_t()
        check(load().he_polyeval_plan(*args, None, 0, C.byref(got)))
        w = (C.c_int64 * got.value)()
        check(load().he_polyeval_plan(*args, w, got.value, C.byref(got)))
        w = [int(x) for x in w]
        self.log_split, self.depth, nl, ns, self.out_level = w[:5]
        self.leaves = [tuple(w[5 + 5 * i: 10 + 5 * i]) for i in range(nl)]
        at = 5 + 5 * nl
        self.steps = [tuple(w[at + 6 * i: at + 6 * i + 6]) for i in range(ns)]

    def log(self):
        """(name, level, degree) per step, the names of the reference's calls (what a trace of the evaluators records)"""
        return [(_OPS[s[0]], s[2], s[3]) for s in self.steps]


# ---- big.Float arithmetic of schemes/ckks/scaling.go, restated on exact rationals ------------------------------------------------
def _round_bits(x, prec: int):
    """x rounded to `prec` significant bits, ties to even: the value a big.Float of that precision holds"""
    x = Fraction(x)
    if x == 0:
        return x
    neg, x = x < 0, abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length() + 1
    if x < Fraction(2) ** (e - 1):
        e -= 1
    ulp = Fraction(2) ** (e - prec)
    m, rem = divmod(x / ulp, 1)
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and int(m) & 1):
        m += 1
    x = int(m) * ulp
    return -x if neg else x


def _big_float_scalar(c, scale, enc_prec: int) -> int:
    """one component of bigComplexToRNSScalar (schemes/ckks/scaling.go:16-40): the constant held at EncodingPrecision, times the
    scale as a 128-bit float, +-0.5 in that precision, truncated"""
    c = _round_bits(c, enc_prec)
    if c == 0:
        return 0
    prec = max(enc_prec, 128)
    r = _round_bits(c * _round_bits(scale, 128), prec)
    r = _round_bits(r + Fraction(1, 2) if c > 0 else r - Fraction(1, 2), prec)
    return math.trunc(r)


def _pair(c):
    if isinstance(c, tuple):
        return Fraction(c[0]), Fraction(c[1])
    if isinstance(c, complex):
        return Fraction(c.real), Fraction(c.imag)
    return Fraction(c), Fraction(0)


class BGVScheme:
    """circuits/bgv/polynomial: scales are residues mod t; a coefficient is an integer mod t"""

    def __init__(self, Q, t: int):
        self.Q, self.t = [int(q) for q in Q], int(t)
        self.tInvModQ, Qi = [], 1  # schemes/bgv/encoder.go:67-71
        for q in self.Q:
            Qi *= q
            self.tInvModQ.append(pow(self.t, -1, Qi))

    def coeff(self, c):
        return int(c) % self.t

    def add(self, a, b):
        return (a + b) % self.t

    def neg(self, a):
        return (-a) % self.t

    def scale(self, s):
        return int(s) % self.t

    def smul(self, a, b):
        return a * b % self.t

    def sdiv(self, a, b):
        return a * pow(int(b) % self.t, -1, self.t) % self.t

    def _centered(self, x):
        x %= self.t
        return x - self.t if x > (self.t >> 1) else x

    def _words(self, level, v):
        w = [v % q for q in self.Q[: level + 1]]
        return w, w

    def const_words(self, level, scale, c):
        """Add with an integer (schemes/bgv/evaluator.go:144-172): at the scale of the ciphertext, centred, times T^-1 mod Q"""
        return self._words(level, self._centered(c * scale) * self.tInvModQ[level])

    def term(self, level, c, xscale, out_scale, earlier):
        """MulThenAdd with an integer (:1108-1140): the op0.Scale != opOut.Scale ratio, centred"""
        v = c
        if xscale != out_scale:
            v *= pow(xscale, self.t - 2, self.t) * out_scale % self.t
        return self._words(level, self._centered(v)), out_scale

    def sub_scale(self, s0, s1):
        if s0 != s1:
            raise ValueError("polyeval: a Chebyshev Sub of operands of different scales needs matchScalesBinary: not supported")
        return s0, None, 1


class CKKSScheme:
    """circuits/ckks/polynomial with LevelsConsumedPerRescaling = 1: scales are exact rationals; a coefficient is a (re, im)
    pair.  imag_unit[i]: the square root of -1 modulo q_i that evaluateWithScalar uses (RootsForward[1], out of Montgomery form:
    ``CKKSScheme.for_ring``)."""

    def __init__(self, Q, imag_unit, default_scale=None):
        self.Q, self.imag_unit, self.t = [int(q) for q in Q], [int(x) for x in imag_unit], None
        self.EncodingPrecision = 53  # Parameters.EncodingPrecision (schemes/ckks/params.go:185-195)
        if default_scale is not None:
            l2 = math.log2(float(default_scale))
            self.EncodingPrecision = 53 if l2 <= 53 else int(l2)

    @classmethod
    def for_ring(cls, ringQ, default_scale=None):
        Q = [int(q) for q in ringQ.ModuliChain()]
        return cls(Q, [int(ringQ.roots(i)[1]) * pow(1 << 64, -1, q) % q for i, q in enumerate(Q)], default_scale)

    def coeff(self, c):
        return _pair(c)

    def add(self, a, b):
        return (a[0] + b[0], a[1] + b[1])

    def neg(self, a):
        return (-a[0], -a[1])

    def scale(self, s):
        return Fraction(s)

    def smul(self, a, b):
        return Fraction(a) * Fraction(b)

    def sdiv(self, a, b):
        return Fraction(a) / Fraction(b)

    def _rns(self, level, scale, c):
        """bigComplexToRNSScalar + the (a + b i, a - b i) pair of evaluateWithScalar (schemes/ckks/scaling.go:10, evaluator.go:410)"""
        re, im = _pair(c)
        real, imag = _big_float_scalar(re, scale, self.EncodingPrecision), _big_float_scalar(im, scale, self.EncodingPrecision)
        s0, s1 = [], []
        for i, q in enumerate(self.Q[: level + 1]):
            r, m = real % q, (imag % q) * self.imag_unit[i] % q
            s0.append((r + m) % q)
            s1.append((r - m) % q)
        return s0, s1

    def _is_int(self, c):
        re, im = _pair(c)
        return _round_bits(re, self.EncodingPrecision).denominator == 1 and _round_bits(im, self.EncodingPrecision).denominator == 1

    def const_words(self, level, scale, c):
        return self._rns(level, scale, c)

    def term(self, level, c, xscale, out_scale, earlier):
        """MulThenAdd with a constant (schemes/ckks/evaluator.go:893-935).  Equal scales and a constant that is no integer: the
        accumulator is first multiplied by q_level (:912-916) -- linear, so it folds into the words of the `earlier` terms"""
        if xscale == out_scale:
            if self._is_int(c):
                scale = 1
            else:
                scale = self.Q[level]
                f0, f1 = self._rns(level, 1, scale)
                for w in earlier:
                    for i, q in enumerate(self.Q[: level + 1]):
                        w[0][i] = w[0][i] * f0[i] % q
                        w[1][i] = w[1][i] * f1[i] % q
                out_scale = out_scale * scale
        elif xscale < out_scale:
            scale = Fraction(out_scale) / Fraction(xscale)
        else:
            raise ValueError("cannot MulThenAdd: op0.Scale > opOut.Scale is not supported")
        return self._rns(level, scale, c), out_scale

    def sub_scale(self, s0, s1):
        """evaluateInPlace (schemes/ckks/evaluator.go:221-400) for op0 - op1 at the scales (s0, s1): the operand of the smaller scale
        is first multiplied by the INTEGER ratio of the two (truncated), and the larger scale is the result's.  Returns (scale,
        which operand is multiplied: 0, 1 or None, the ratio)"""
        if s0 == s1:
            return s0, None, 1
        if s0 > s1:
            return s0, 1, int(Fraction(s0) / Fraction(s1))
        return s1, 0, int(Fraction(s1) / Fraction(s0))

    def ratio_words(self, level, ratio):
        """Mul by the integer ratio (:625-660): an integer constant is encoded at scale 1"""
        return self._rns(level, 1, (Fraction(ratio), Fraction(0)))


class Polynomial:
    """polynomial.Polynomial over bignum.Polynomial (circuits/common/polynomial/polynomial.go:12-30): Coeffs[i] may be None where
    the parity excludes index i; IsEven and IsOdd both set (bignum.NewPolynomial) or both clear: no parity filter"""

    def __init__(self, coeffs, Basis="Monomial", IsEven=True, IsOdd=True, Lazy=False):
        self.Coeffs, self.Basis, self.IsEven, self.IsOdd, self.Lazy = list(coeffs), Basis, bool(IsEven), bool(IsOdd), bool(Lazy)

    def Degree(self):
        return len(self.Coeffs) - 1

    def Depth(self):
        return Depth(self.Degree())

    def _wanted(self, i):
        return True if not (self.IsEven or self.IsOdd) else (self.IsEven if i % 2 == 0 else self.IsOdd)

    def Plan(self, scheme, level: int, scale, target_scale, powers=None, ring=None, copy_input=True) -> "PlannedPolynomial":
        """plan levels, scales and scalar words for an input at (level, scale) -- or for a basis that already holds `powers`
        ({n: (level, degree, scale)}, X^1 among them) -- and the scale the result shall have.  With `ring` (a lattigo_amd Ring)
        the native Polynomial is created and the words uploaded; without, the planning alone (no device needed)."""
        return PlannedPolynomial(self, scheme, level, scale, target_scale, powers, ring, copy_input)


def _walk_powers(sc, steps, pscale, plevel):
    """the scales of the powers as the plan's steps make them (pscale / plevel are updated): (the scale after every power step,
    the Add(x, -1) steps as (step, power, level, s0, s1), the Subs whose operands differ in scale as (step, dst, a, which operand
    is multiplied first, the integer ratio, level, s0, s1), the index of the first step that is no power step)"""
    Q, scales, minus_one, sub_ratio = sc.Q, [], [], []
    for i, (op, dst, lvl, deg, a, b) in enumerate(steps):
        if op >= OP_NEW or dst < 0:
            return scales, minus_one, sub_ratio, i
        if op == OP_RESCALE:
            pscale[dst] = sc.sdiv(pscale[dst], Q[lvl + 1])
        elif op in (OP_MUL_NEW, OP_MUL_RELIN_NEW):
            pscale[dst] = sc.smul(pscale[a], pscale[b])
        elif op == OP_ADD_MINUS_ONE:
            minus_one.append((i, dst, lvl) + tuple(sc.const_words(lvl, pscale[dst], sc.coeff(-1))))
        elif op == OP_SUB:
            pscale[dst], which, ratio = sc.sub_scale(pscale[dst], pscale[a])
            if which is not None:  # (a ratio of 1 included: the reference multiplies by it all the same)
                sub_ratio.append((i, dst, a, which, ratio, lvl) + tuple(sc.ratio_words(lvl, ratio)))
        plevel[dst] = lvl
        scales.append(pscale[dst])
    return scales, minus_one, sub_ratio, len(steps)


class PlannedPolynomial:
    """.plan: the library's Plan; .scales: the scale of the destination after every step of it; .leaves: per baby step
    dict(degree, level, scale, out_scale, coeffs, words = [(k, s0, s1)] in the reference's order: the constant, then k = deg ...
    1); .minus_one: per Add(x, -1) step of the plan, (step, power, level, s0, s1);
    .sub_ratio: per Chebyshev Sub whose operands differ in scale, (step, dst, a, which operand is multiplied first: 0 = dst, 1 = a,
    the integer ratio, level, s0, s1); .out_scale / .out_level: of the result"""

    def __init__(self, pol: Polynomial, scheme, level, scale, target_scale, powers, ring, copy_input):
        sc = self.scheme = scheme
        self.pol = pol
        if powers is None:
            powers = {1: (int(level), 1, scale)}
        self.plan = Plan(pol.Degree(), pol.Basis, pol.IsEven, pol.IsOdd, pol.Lazy, {n: (v[0], v[1]) for n, v in powers.items()}, copy_input=copy_input)
        level, scale = powers[1][0], sc.scale(powers[1][2])
        self.level = level
        target_scale = sc.scale(target_scale)
        Q = sc.Q
        # -- the powers as the steps make them
        pscale = {n: sc.scale(v[2]) for n, v in powers.items()}
        plevel = {n: v[0] for n, v in powers.items()}
        self.scales, self.minus_one, self.sub_ratio, first_leaf = _walk_powers(sc, self.plan.steps, pscale, plevel)
        self.power_scales, self.power_levels = pscale, plevel
        # -- the decomposition: coefficients, levels and scales of the baby steps (polynomial.go:62-141 with the simulated
        # evaluators of circuits/{bgv,ckks}/polynomial/polynomial_evaluator_sim.go)
        d = pol.Degree()
        log_degree = d.bit_length()
        sim = {1: (level, scale)}

        def sim_power(n):  # SimPowerBasis.GenPower: recomputed on every visit, like the reference
            if n < 2:
                return
            a, b = SplitDegree(n)
            sim_power(a)
            sim_power(b)
            la, sa = sim[a]
            lb, sb = sim[b]
            lm = min(la, lb)
            sim[n] = (lm - 1, sc.sdiv(sc.smul(sa, sb), Q[lm]))

        sim_power(1 << log_degree)
        for i in range((1 << self.plan.log_split) - 1, 2, -1):
            sim_power(i)
        leaves = []
        coeffs = [None if c is None else sc.coeff(c) for c in pol.Coeffs]

        def split(c, n, lead, maxdeg):
            dd = len(c) - 1
            r, q = list(c[:n]), [None] * (dd - n + 1)
            q[0] = c[n]
            for i in range(n + 1, dd + 1):
                if c[i] is None or not pol._wanted(i):
                    continue
                if pol.Basis == "Chebyshev":  # T_i = 2 T_n T_{i-n} - T_{2n-i}
                    q[i - n] = sc.add(c[i], c[i])
                    r[2 * n - i] = sc.add(r[2 * n - i], sc.neg(c[i])) if r[2 * n - i] is not None else sc.neg(c[i])
                else:
                    q[i - n] = c[i]
            return (q, lead, maxdeg), (r, False, (n - 1) if maxdeg == dd else maxdeg - (dd - n + 1))

        def descend(c, lead, maxdeg, ls, lvl, out_scale):
            dd = len(c) - 1
            if dd < (1 << ls):
                if lead and ls > 1 and maxdeg > (1 << maxdeg.bit_length()) - (1 << (ls - 1)):
                    return descend(c, lead, maxdeg, OptimalSplit(dd.bit_length()), lvl, out_scale)
                s = sc.smul(out_scale, Q[lvl]) if lead else out_scale  # UpdateLevelAndScaleBabyStep
                leaves.append(dict(degree=dd, level=lvl, scale=s, coeffs=c))
                return lvl, s
            step = 1 << ls
            while step < (dd >> 1) + 1:
                step <<= 1
            (cq, lq, mq), (cr, lr, mr) = split(c, step, lead, maxdeg)
            qi = Q[lvl] if lead else Q[lvl + 1]  # UpdateLevelAndScaleGiantStep
            tl, ts = descend(cq, lq, mq, ls, lvl + 1, sc.sdiv(sc.smul(out_scale, qi), sim[step][1]))
            tl, ts = min(tl - 1, sim[step][0]), sc.smul(sc.sdiv(ts, Q[tl]), sim[step][1])
            _, rs = descend(cr, lr, mr, ls, lvl, ts)
            if rs != ts:
                raise RuntimeError(f"recursePS: res.Scale != tmp.Scale: {ts} != {rs}")
            return tl, ts

        descend(coeffs, True, d, self.plan.log_split, level - (log_degree - 1), target_scale)
        if [(f["degree"], f["level"]) for f in leaves] != [(f[0], f[1]) for f in self.plan.leaves]:
            raise RuntimeError("polyeval: the planned baby steps differ from the library's decomposition")
        # -- the words of every baby step, in the order of the reference's calls
        for f, pf in zip(leaves, self.plan.leaves):
            out_scale, words, after = f["scale"], [], []
            if pf[4] & 1:
                words.append((0,) + tuple(list(w) for w in sc.const_words(f["level"], out_scale, f["coeffs"][0])))
                after.append(out_scale)
            for k in range(f["degree"], 0, -1):
                if (pf[4] >> k) & 1:
                    w, out_scale = sc.term(f["level"], f["coeffs"][k], pscale[k], out_scale, [x[1:] for x in words])
                    words.append((k, list(w[0]), list(w[1])))
                    after.append(out_scale)
            f["words"], f["out_scale"], f["ct_degree"], f["after"] = words, out_scale, pf[3], after
        self.leaves = leaves
        # -- the giant steps
        lscale = {-1 - i: f["out_scale"] for i, f in enumerate(leaves)}
        for op, dst, lvl, deg, a, b in self.plan.steps[first_leaf:]:
            if op == OP_NEW:  # (a new ciphertext carries the scale 1 until the evaluator sets the baby step's)
                self.scales.append(sc.scale(1))
                seen = iter(leaves[-1 - dst]["after"])
                continue
            if op in (OP_ADD_CONST, OP_MUL_THEN_ADD):
                self.scales.append(next(seen))
                continue
            if op == OP_RESCALE:
                lscale[dst] = sc.sdiv(lscale[dst], Q[lvl + 1])
            elif op == OP_MUL:
                lscale[dst] = sc.smul(lscale[dst], pscale[a])
            elif op == OP_ADD and lscale[dst] != lscale[a]:
                raise RuntimeError(f"evalMonomial: scale discrepency: (rescale(b) * X^{{n}}).Scale = {lscale[dst]} != a.Scale = {lscale[a]}")
            self.scales.append(lscale[dst])
        self.out_scale, self.out_level = lscale[self.plan.steps[-1][1]], self.plan.out_level
        self.result = self.plan.steps[-1][1]
        self._powers0 = {n: (v[0], v[1]) for n, v in powers.items()}
        self.h, self._group = None, 0
        if ring is not None:
            self._create(ring)

    def _create(self, ring):
        L = self.level + 1
        rows0, rows1 = [], []
        for f in self.leaves:
            by_k = {k: (s0, s1) for k, s0, s1 in f["words"]}
            for k in range(f["degree"] + 1):
                s0, s1 = by_k.get(k, ([], []))
                rows0.append(list(s0) + [0] * (L - len(s0)))
                rows1.append(list(s1) + [0] * (L - len(s1)))
        s0 = np.ascontiguousarray(np.array(rows0, dtype=np.uint64))
        s1 = np.ascontiguousarray(np.array(rows1, dtype=np.uint64))
        pol = self.pol
        flat, n = _ints([v for k in sorted(self._powers0) for v in (k,) + self._powers0[k]])
        deg, _ = _ints([f["degree"] for f in self.leaves])
        lvl, _ = _ints([f["level"] for f in self.leaves])
        h = H()
        check(load().he_polyeval_poly_create(ring.h, pol.Degree(), 1 if pol.Basis == "Chebyshev" else 0, int(pol.IsEven), int(pol.IsOdd),
                                             int(pol.Lazy), n // 3, flat, len(self.leaves), deg, lvl, s0.ctypes.data_as(u64p),
                                             s1.ctypes.data_as(u64p), C.byref(h)))
        self.h, self.ring = h.value, ring

    def SetGroup(self, G: int):
        """baby steps per launch of the leaf-group kernel: 0 (the library's default), 1, 2 or 4"""
        check(load().he_polyeval_poly_set_group(self.h, int(G)))

    def EvaluatePolynomialFromPowerBasis(self, X: dict, out, first: int = 0, count: int | None = None):
        """EvaluatePolynomialVectorFromPowerBasis (polynomial_evaluator.go:254-359) for the baby steps [first, first + count):
        X = {k: [Poly per component of X^k]}; out[g] = the list of polynomials of baby step first + g's result, exactly
        ``self.leaves[first + g]["ct_degree"] + 1`` of them, each of at least that baby step's level + 1 limbs"""
        count = len(self.leaves) - first if count is None else count
        top = max([f["degree"] for f in self.leaves[first: first + count]] + [0])
        xs = (H * max(3 * top, 1))()
        for k in range(1, top + 1):
            for c, p in enumerate(X.get(k, [])):
                xs[3 * (k - 1) + c] = p.h
        os_ = (H * (3 * count))()
        for g in range(count):
            for c, p in enumerate(out[g]):
                os_[3 * g + c] = p.h
        check(load().he_polyeval_leaves(self.h, first, count, top, xs, os_))
        return out

    def __del__(self):
        try:
            if getattr(self, "h", None):
                load().he_polyeval_poly_destroy(self.h)
                self.h = None
        except Exception:
            pass


# ---- polynomial.Evaluator: one native call per evaluation -----------------------------------------------------------------------------
class Ciphertext:
    """rlwe.Ciphertext: Value = degree + 1 device polynomials (NTT domain), Level, Scale (a residue mod t for BGV, an exact
    rational for CKKS)"""

    def __init__(self, value, level: int, scale):
        self.Value, self.level, self.Scale = list(value), int(level), scale

    def Degree(self):
        return len(self.Value) - 1

    def Level(self):
        return self.level


def _aux(pl, first=0):
    """the Chebyshev numbers of the plan's steps, in its order: (n, kinds, s0, s1, words per entry)"""
    minus_one = {m[0]: m for m in pl.minus_one}
    ratios = {r[0]: r for r in pl.sub_ratio}
    L = pl.level + 1
    kinds, r0, r1 = [], [], []
    for i, st in enumerate(pl.plan.steps):
        if i < first or st[0] not in (OP_ADD_MINUS_ONE, OP_SUB):
            continue
        if st[0] == OP_ADD_MINUS_ONE:
            kind, w0, w1 = 0, minus_one[i][3], minus_one[i][4]
        elif i in ratios:
            kind, w0, w1 = (1 if ratios[i][3] == 1 else 2), ratios[i][6], ratios[i][7]
        else:
            kind, w0, w1 = 3, [], []
        kinds.append(kind)
        r0.append(list(w0) + [0] * (L - len(w0)))
        r1.append(list(w1) + [0] * (L - len(w1)))
    n = len(kinds)
    s0 = np.ascontiguousarray(np.array(r0 or [[0] * L], dtype=np.uint64))
    s1 = np.ascontiguousarray(np.array(r1 or [[0] * L], dtype=np.uint64))
    return n, _ints(kinds)[0], s0, s1, L


class PowerBasis:
    """polynomial.PowerBasis (power_basis.go:17-29) on the device (he_polyeval_basis_*): NewPowerBasis copies the input into X^1.
    The polynomials live in the library; ``Scale[n]`` is kept here, where the scales are planned."""

    def __init__(self, evaluator, ct: Ciphertext, Basis="Monomial"):
        if ct.Degree() != 1:
            raise ValueError("PowerBasis: a ciphertext of degree 1 is expected")
        self.eval, self.Basis, self.Scale = evaluator, Basis, {1: ct.Scale}
        h = H()
        check(load().he_polyeval_basis_create(evaluator.h, 1 if Basis == "Chebyshev" else 0, ct.level, ct.Value[0].h, ct.Value[1].h, C.byref(h)))
        self.h = h.value

    def Powers(self) -> dict:
        """{n: (level, ciphertext degree)} of the powers the basis holds"""
        n = C.c_size_t()
        check(load().he_polyeval_basis_powers(self.h, None, 0, C.byref(n)))
        out = (C.c_int * (3 * max(n.value, 1)))()
        check(load().he_polyeval_basis_powers(self.h, out, n.value, C.byref(n)))
        return {int(out[3 * i]): (int(out[3 * i + 1]), int(out[3 * i + 2])) for i in range(n.value)}

    def held(self) -> dict:
        return {n: (lv, dg, self.Scale[n]) for n, (lv, dg) in self.Powers().items()}

    def Words(self, n: int) -> np.ndarray:
        """the words of X^n, [batch][degree + 1][limbs][N] (tests)"""
        comps = (H * 3)()
        check(load().he_polyeval_basis_power(self.h, int(n), comps))
        out = []
        for c in range(3):
            if comps[c]:
                nl, b, nn = C.c_int(), C.c_int(), C.c_int()
                check(load().he_poly_shape(comps[c], C.byref(nl), C.byref(b), C.byref(nn)))
                a = np.empty((b.value, nl.value, nn.value), dtype=np.uint64)
                check(load().he_poly_download(comps[c], a.ctypes.data_as(u64p), a.size))
                out.append(a)
        return np.stack(out, axis=1)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                load().he_polyeval_basis_destroy(self.h)
                self.h = None
        except Exception:
            pass


class Evaluator:
    """polynomial.Evaluator (circuits/common/polynomial/polynomial_evaluator.go) for BGV (`scheme` a BGVScheme) or CKKS (a
    CKKSScheme): Evaluate and EvaluateFromPowerBasis are ONE native call each (he_polyeval_evaluate[_from_power_basis]), GenPower
    likewise.  What this class adds is the planning: scales and scalar words, the planned polynomial kept per (polynomial, basis,
    target) -- at most `cache` of them, the least recently used released first -- so that its words are uploaded once."""

    def __init__(self, evaluator, scheme, rlk=None, cache: int = 16):
        self.eval, self.scheme, self.rlk, self.ringQ = evaluator, scheme, rlk, evaluator.ringQ
        self.bgv = scheme.t is not None
        self.group, self._plans, self._cache = 0, {}, max(int(cache), 1)

    def SetGroup(self, G: int):
        """baby steps per launch of the leaf-group kernel: 0 (the library's default), 1, 2 or 4"""
        self.group = int(G)
        for pl in self._plans.values():
            pl.SetGroup(self.group)

    def NewPowerBasis(self, ct: Ciphertext, Basis="Monomial") -> PowerBasis:
        return PowerBasis(self.eval, ct, Basis)

    def _planned(self, held, pol, target):
        key = (tuple(pol.Coeffs), pol.Basis, pol.IsEven, pol.IsOdd, pol.Lazy, tuple(sorted(held.items())), target)
        pl = self._plans.pop(key, None)
        if pl is None:
            pl = pol.Plan(self.scheme, held[1][0], held[1][2], target, powers=held, ring=self.ringQ, copy_input=False)
            pl.SetGroup(self.group)
        self._plans[key] = pl  # (most recently used last)
        while len(self._plans) > self._cache:
            self._plans.pop(next(iter(self._plans)))
        return pl

    def _scheme_args(self):
        return (1 if self.bgv else 0, self.scheme.t or 0, self.rlk.h if self.rlk is not None else 0)

    def _result(self, pl, batch):
        from lattigo_amd.ring import Poly
        if pl.out_level < 0:
            raise ValueError("polyeval: the result would sink below level 0")
        return Ciphertext([Poly(self.ringQ, pl.out_level + 1, batch, zero=False) for _ in range(2)], pl.out_level, pl.out_scale)

    def Evaluate(self, ct: Ciphertext, pol: Polynomial, targetScale) -> Ciphertext:
        """Evaluator.Evaluate (:33-99) on a ciphertext: the input is left untouched"""
        Depth(pol.Degree(), ct.level)  # the reference's error, before anything is planned
        pl = self._planned({1: (ct.level, 1, ct.Scale)}, pol, targetScale)
        res = self._result(pl, ct.Value[0].batch)
        n, kinds, s0, s1, L = _aux(pl)
        check(load().he_polyeval_evaluate(self.eval.h, pl.h, *self._scheme_args(), ct.level, ct.Value[0].h, ct.Value[1].h, n, kinds,
                                          s0.ctypes.data_as(u64p), s1.ctypes.data_as(u64p), L, res.Value[0].h, res.Value[1].h))
        return res

    def EvaluateFromPowerBasis(self, pb: PowerBasis, pol: Polynomial, targetScale) -> Ciphertext:
        """Evaluator.EvaluateFromPowerBasis (:47-99): powers the basis lacks are generated into it"""
        if pb.Basis != pol.Basis:
            raise ValueError("cannot EvaluateFromPowerBasis: the polynomial and the power basis differ in basis")
        pl = self._planned(pb.held(), pol, targetScale)
        res = self._result(pl, self._batch(pb))
        n, kinds, s0, s1, L = _aux(pl)
        check(load().he_polyeval_evaluate_from_power_basis(pb.h, pl.h, *self._scheme_args(), n, kinds, s0.ctypes.data_as(u64p),
                                                           s1.ctypes.data_as(u64p), L, res.Value[0].h, res.Value[1].h))
        pb.Scale.update({k: v for k, v in pl.power_scales.items()})
        return res

    def GenPower(self, pb: PowerBasis, n: int, lazy: bool = False):
        """PowerBasis.GenPower (power_basis.go:76-160) as one native call; the scales follow the steps the library lists"""
        held = pb.held()
        flat, cnt = _ints([v for k in sorted(held) for v in (k, held[k][0], held[k][1])])
        args = (1 if pb.Basis == "Chebyshev" else 0, int(n), int(bool(lazy)), cnt // 3, flat)
        got = C.c_size_t()
        check(load().he_polyeval_gen_power_plan(*args, None, 0, C.byref(got)))
        w = (C.c_int64 * max(got.value, 1))()
        check(load().he_polyeval_gen_power_plan(*args, w, got.value, C.byref(got)))
        steps = [tuple(int(x) for x in w[6 * i: 6 * i + 6]) for i in range(got.value // 6)]

        class run:  # what _aux reads
            pass
        run.plan = type("steps", (), {"steps": steps})
        run.level = held[1][0]
        pscale = {k: self.scheme.scale(v[2]) for k, v in held.items()}
        _, run.minus_one, run.sub_ratio, _ = _walk_powers(self.scheme, steps, pscale, {k: v[0] for k, v in held.items()})
        cnt, kinds, s0, s1, L = _aux(run)
        check(load().he_polyeval_gen_power(pb.h, *self._scheme_args(), int(n), int(bool(lazy)), cnt, kinds, s0.ctypes.data_as(u64p),
                                           s1.ctypes.data_as(u64p), L))
        pb.Scale.update(pscale)

    @staticmethod
    def _batch(pb):
        comps = (H * 3)()
        check(load().he_polyeval_basis_power(pb.h, 1, comps))
        nl, b, nn = C.c_int(), C.c_int(), C.c_int()
        check(load().he_poly_shape(comps[0], C.byref(nl), C.byref(b), C.byref(nn)))
        return b.value
