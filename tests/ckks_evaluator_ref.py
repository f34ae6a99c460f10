"""The four entries of include/hering_ckks_evaluator.h restated as the reference's own sequences of ring operations
(schemes/ckks/evaluator.go, cited per function) over oracle/oracle.py's ring primitives, one batch entry at a time, and -- apart
from it -- as plain modular arithmetic on Python integers (`exact_*`): the first is held against the second without a device in
tests/test_ckks_evaluator_host.py, the device against both in tests/test_gpu_ckks_evaluator.py.

A ciphertext is a list of [limbs][N] uint64 arrays (its components); every function works on copies of the pre-call words.

rlwe.Scale is restated here as `Scale` with integers only (a 128-bit mantissa and a binary exponent): the second, independent
restatement that lattigo_amd.rlwe.Scale is held against."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from oracle import oracle as O

PREC = 128  # rlwe.ScalePrecision (core/rlwe/scale.go:17)


# ---- rlwe.Scale: big.Float of 128 bits, round to nearest even (core/rlwe/scale.go) -------------------------------------------------
def _round_mant(num: int, den: int):
    """(m, e) with m * 2^e = num / den rounded to PREC bits, nearest even; num, den > 0"""
    e = num.bit_length() - den.bit_length() - PREC
    while True:
        n, d = (num, den << e) if e >= 0 else (num << -e, den)
        m, r = divmod(n, d)
        if m.bit_length() > PREC:
            e += 1
            continue
        if m.bit_length() < PREC:
            e -= 1
            continue
        break
    if 2 * r > d or (2 * r == d and (m & 1)):
        m += 1
        if m.bit_length() > PREC:
            m >>= 1
            e += 1
    return m, e


class Scale:
    """value = m * 2^e with m < 2^128 (0: the zero scale)"""

    def __init__(self, v=0):
        if isinstance(v, Scale):
            self.m, self.e = v.m, v.e
            return
        f = Fraction(v)  # ints and float64 are exact
        if f < 0:
            raise ValueError("a scale is not negative")
        self.m, self.e = (0, 0) if f == 0 else _round_mant(f.numerator, f.denominator)

    @classmethod
    def _of(cls, m, e):
        s = cls()
        s.m, s.e = m, e
        return s

    def fraction(self) -> Fraction:
        return Fraction(self.m) * (Fraction(2) ** self.e)

    def Mul(self, o):
        f = self.fraction() * Scale(o).fraction()
        return Scale._of(*((0, 0) if f == 0 else _round_mant(f.numerator, f.denominator)))

    def Div(self, o):
        f = self.fraction() / Scale(o).fraction()
        return Scale._of(*((0, 0) if f == 0 else _round_mant(f.numerator, f.denominator)))

    def Cmp(self, o) -> int:
        a, b = self.fraction(), Scale(o).fraction()
        return (a > b) - (a < b)

    def Max(self, o):
        return Scale(self) if self.Cmp(o) >= 0 else Scale(o)

    def Min(self, o):
        return Scale(self) if self.Cmp(o) <= 0 else Scale(o)

    def Int(self) -> int:  # big.Float.Int: truncation
        return (self.m << self.e) if self.e >= 0 else (self.m >> -self.e)

    def Float64(self) -> float:  # nearest even: Python's int / int true division is correctly rounded
        f = self.fraction()
        return f.numerator / f.denominator


# ---- the entries over the oracle's ring primitives ---------------------------------------------------------------------------------
def _ring(ring: O.Ring, level: int) -> O.Ring:
    return ring if level == ring.MaxLevel() else O.Ring(ring.N, ring.moduli[: level + 1])


def _mul_int(r: O.Ring, ct, words):
    """Evaluator.Mul(ct, ratioInt, tmp) (:629-666): the scalar is an integer, MulDoubleRNSScalar with both halves alike"""
    return [r.MulDoubleRNSScalar(c, words, words) for c in ct]


def ckks_add(ring: O.Ring, level: int, sub: bool, op0, op1, scaled: int = 0, ratio=None):
    """evaluateInPlace (:221-408) and the Neg of Sub (:152-156)"""
    r = _ring(ring, level)
    t0 = [np.array(c[: level + 1], dtype=np.uint64) for c in op0]
    t1 = [np.array(c[: level + 1], dtype=np.uint64) for c in op1]
    if scaled == 1:
        t0 = _mul_int(r, t0, ratio)
    elif scaled == 2:
        t1 = _mul_int(r, t1, ratio)
    lo = min(len(t0), len(t1))
    out = [r.binop("Sub" if sub else "Add", t0[i], t1[i]) for i in range(lo)]
    out += [c.copy() for c in t0[lo:]]                                  # :399-402 CopyLvl
    out += [r.unop("Neg", c) if sub else c.copy() for c in t1[lo:]]     # :403-406 CopyLvl, :152-156 Neg
    return out


def ckks_scalar(ring: O.Ring, level: int, op: int, op0, s0, s1, out=None, pre=None):
    """evaluateWithScalar (:410-424) after its preparation loop"""
    r = _ring(ring, level)
    x = [np.array(c[: level + 1], dtype=np.uint64) for c in op0]
    if op == 0:
        return [r.AddDoubleRNSScalar(x[0], s0, s1)] + [c.copy() for c in x[1:]]     # :80-86
    if op == 1:
        return [r.SubDoubleRNSScalar(x[0], s0, s1)] + [c.copy() for c in x[1:]]     # :171-177
    if op == 2:
        return [r.MulDoubleRNSScalar(c, s0, s1) for c in x]                         # :661
    acc = [np.array(c[: level + 1], dtype=np.uint64) for c in out]
    if pre is not None:
        acc = _mul_int(r, acc, pre)                                                 # :959-964
    return [r.MulDoubleRNSScalarThenAdd(c, s0, s1, a) for c, a in zip(x, acc)]      # :975


def ckks_mul_pt(ring: O.Ring, level: int, ct, pt, out=None, pre=None):
    r = _ring(ring, level)
    x = [np.array(c[: level + 1], dtype=np.uint64) for c in ct]
    c00 = r.unop("MForm", np.array(pt[: level + 1], dtype=np.uint64))               # :860 / :1166
    if out is None:
        return [r.binop("MulCoeffsMontgomery", c00, c) for c in x]                  # :866-868
    acc = [np.array(c[: level + 1], dtype=np.uint64) for c in out]
    if pre is not None:
        acc = _mul_int(r, acc, pre)                                                 # :1087-1096
    return [r.binop("MulCoeffsMontgomeryThenAdd", c, c00, a) for c, a in zip(x, acc)]  # :1167-1169


def ckks_mul_relin_then_add(ring: O.Ring, level: int, a, b, out, pre=None, oev: O.Evaluator | None = None, rlk=None):
    """the ciphertext x ciphertext branch of mulRelinThenAdd (:1104-1155); with oev and rlk: the relinearizing form"""
    r = _ring(ring, level)
    a = [np.array(c[: level + 1], dtype=np.uint64) for c in a]
    b = [np.array(c[: level + 1], dtype=np.uint64) for c in b]
    acc = [np.array(c[: level + 1], dtype=np.uint64) for c in out]
    if pre is not None:
        acc = _mul_int(r, acc, pre)
    c00, c01 = r.unop("MForm", a[0]), r.unop("MForm", a[1])                         # :1128-1129
    c0 = r.binop("MulCoeffsMontgomeryThenAdd", c00, b[0], acc[0])                   # :1131
    c1 = r.binop("MulCoeffsMontgomeryThenAdd", c00, b[1], acc[1])                   # :1132
    c1 = r.binop("MulCoeffsMontgomeryThenAdd", c01, b[0], c1)                       # :1133
    if rlk is None:
        return [c0, c1, r.binop("MulCoeffsMontgomeryThenAdd", c01, b[1], acc[2])]   # :1154
    c2 = r.binop("MulCoeffsMontgomery", c01, b[1])                                  # :1143
    t = oev.GadgetProduct(level, c2, rlk)                                           # :1150
    return [r.binop("Add", c0, t[0][: level + 1]), r.binop("Add", c1, t[1][: level + 1])]  # :1151-1152


# ---- the same as plain arithmetic ------------------------------------------------------------------------------------------------------
def _obj(c, level):
    return np.array(c[: level + 1], dtype=np.uint64).astype(object)


def _mods(ring, level):
    return np.array([int(m) for m in ring.moduli[: level + 1]], dtype=object)[:, None]


def _u64(x):
    return np.array(x, dtype=np.uint64)


def exact_add(ring, level, sub, op0, op1, scaled=0, ratio=None):
    q = _mods(ring, level)
    rr = np.array([int(w) for w in ratio[: level + 1]], dtype=object)[:, None] if scaled else 1
    t0 = [(_obj(c, level) * (rr if scaled == 1 else 1)) % q for c in op0]
    t1 = [(_obj(c, level) * (rr if scaled == 2 else 1)) % q for c in op1]
    lo = min(len(t0), len(t1))
    out = [_u64((t0[i] - t1[i]) % q if sub else (t0[i] + t1[i]) % q) for i in range(lo)]
    out += [_u64(c) for c in t0[lo:]]
    out += [_u64(q - c if sub else c) for c in t1[lo:]]  # Ring.Neg: q - x, q for a zero
    return out


def _halves(ring, level, s0, s1):
    h = ring.N // 2
    s = np.empty((level + 1, ring.N), dtype=object)
    for i in range(level + 1):
        s[i, :h], s[i, h:] = int(s0[i]), int(s1[i])
    return s


def exact_scalar(ring, level, op, op0, s0, s1, out=None, pre=None):
    q, s = _mods(ring, level), _halves(ring, level, s0, s1)
    x = [_obj(c, level) for c in op0]
    if op in (0, 1):
        return [_u64((x[0] - s) % q if op else (x[0] + s) % q)] + [_u64(c) for c in x[1:]]
    if op == 2:
        return [_u64(c * s % q) for c in x]
    pp = np.array([int(w) for w in pre[: level + 1]], dtype=object)[:, None] if pre is not None else 1
    return [_u64((_obj(a, level) * pp + c * s) % q) for c, a in zip(x, out)]


def exact_mul_pt(ring, level, ct, pt, out=None, pre=None):
    q, m = _mods(ring, level), _obj(pt, level)
    if out is None:
        return [_u64(_obj(c, level) * m % q) for c in ct]
    pp = np.array([int(w) for w in pre[: level + 1]], dtype=object)[:, None] if pre is not None else 1
    return [_u64((_obj(a, level) * pp + _obj(c, level) * m) % q) for c, a in zip(ct, out)]


def exact_mul_then_add(ring, level, a, b, out, pre=None):
    q = _mods(ring, level)
    a0, a1, b0, b1 = (_obj(c, level) for c in (a[0], a[1], b[0], b[1]))
    pp = np.array([int(w) for w in pre[: level + 1]], dtype=object)[:, None] if pre is not None else 1
    acc = [_obj(c, level) * pp for c in out]
    return [_u64((acc[0] + a0 * b0) % q), _u64((acc[1] + a0 * b1 + a1 * b0) % q), _u64((acc[2] + a1 * b1) % q)]


# ---- ckks.Evaluator with metadata, line by line (schemes/ckks/evaluator.go) ---------------------------------------------------------------
def _bigfloat(x, prec: int) -> Fraction:
    """the value a big.Float of `prec` bits holds after x is stored in it (nearest even), by integers"""
    x = Fraction(x)
    if x == 0:
        return x
    num, den = abs(x.numerator), x.denominator
    e = num.bit_length() - den.bit_length() - prec
    while True:
        n, d = (num, den << e) if e >= 0 else (num << -e, den)
        m, r = divmod(n, d)
        if m.bit_length() > prec:
            e += 1
        elif m.bit_length() < prec:
            e -= 1
        else:
            break
    if 2 * r > d or (2 * r == d and (m & 1)):
        m += 1
    v = Fraction(m) * Fraction(2) ** e
    return -v if x < 0 else v


def _parts(c):
    if isinstance(c, complex):
        return Fraction(c.real), Fraction(c.imag)
    return Fraction(c), Fraction(0)


class RefCt:
    """rlwe.Ciphertext / Plaintext on the host: Value = components [limbs][N]; MetaData = (Scale, LogSlots)"""

    def __init__(self, value, scale, log_slots=None):
        self.Value = [np.array(v, dtype=np.uint64) for v in value]
        self.Scale = Scale(scale)
        self.LogSlots = log_slots

    def Level(self):
        return self.Value[0].shape[0] - 1

    def Degree(self):
        return len(self.Value) - 1

    def Resize(self, degree, level):
        N = self.Value[0].shape[1]
        self.Value = [v[: level + 1] if v.shape[0] >= level + 1 else np.concatenate([v, np.zeros((level + 1 - v.shape[0], N), dtype=np.uint64)])
                      for v in self.Value[: degree + 1]]
        while len(self.Value) < degree + 1:
            self.Value.append(np.zeros((level + 1, N), dtype=np.uint64))

    def CopyNew(self):
        return RefCt([v.copy() for v in self.Value], self.Scale, self.LogSlots)


class RefEvaluator:
    """the reference's evaluator over the oracle's ring primitives; `encode(values, level, scale) -> [limbs][N]` serves the vector
    operands (Encoder.Encode)"""

    def __init__(self, oev: O.Evaluator, default_scale, rlk=None, gks=None, encode=None):
        import math
        self.oev, self.ringQ, self.rlk, self.gks, self.encode = oev, oev.ringQ, rlk, gks or {}, encode
        self.Q = [int(q) for q in oev.ringQ.moduli]
        self.default_scale = Scale(default_scale)
        l2 = math.log2(Scale(default_scale).Float64())
        self.prec = 53 if l2 <= 53 else int(l2)  # Parameters.EncodingPrecision (params.go:185-195)

    def NewCiphertext(self, degree, level):
        return RefCt([np.zeros((level + 1, self.ringQ.N), dtype=np.uint64) for _ in range(degree + 1)], self.default_scale)  # ckks.NewCiphertext

    def _r(self, level):
        return _ring(self.ringQ, level)

    # bignum.ToComplex + bigComplexToRNSScalar (scaling.go:10-43) + the loop of evaluateWithScalar (:416-419)
    def _is_int(self, c):
        return all(_bigfloat(p, self.prec).denominator == 1 for p in _parts(c))

    def _rns(self, level, scale: "Scale", c):
        out = []
        for part in _parts(c):
            v = _bigfloat(part, self.prec)
            if v == 0:
                out.append(0)
                continue
            prec = max(self.prec, PREC)
            r = _bigfloat(v * scale.fraction(), prec)
            r = _bigfloat(r + Fraction(1, 2) if v > 0 else r - Fraction(1, 2), prec)
            out.append(int(r) if r >= 0 else -int(-r))  # big.Float.Int truncates towards zero
        s0, s1 = [], []
        for i, q in enumerate(self.Q[: level + 1]):
            re, im = out[0] % q, O.MRed(out[1] % q, int(self.ringQ.roots_forward(i)[1]), q)
            s0.append((re + im) % q)
            s1.append((re + q - im) % q)
        return np.array(s0, dtype=np.uint64), np.array(s1, dtype=np.uint64)

    def _is_scalar(self, x):
        return isinstance(x, (int, float, complex, Fraction)) and not isinstance(x, bool)

    def _pt(self, values, level, like, scale):
        return RefCt([self.encode(values, level, Scale(scale).Float64())], scale, like.LogSlots)

    # -- Add / Sub (:51-219)
    def _addsub(self, op0, op1, opOut, sub):
        if self._is_scalar(op1):
            level = min(op0.Level(), opOut.Level())
            opOut.Resize(op0.Degree(), level)
            s0, s1 = self._rns(level, op0.Scale, op1)
            r = self._r(level)
            head = (r.SubDoubleRNSScalar if sub else r.AddDoubleRNSScalar)(op0.Value[0][: level + 1], s0, s1)
            if op0 is not opOut:
                for i in range(1, len(opOut.Value)):
                    opOut.Value[i] = op0.Value[i][: level + 1].copy()
            opOut.Value[0] = head  # (the scale of opOut is not touched: neither InitOutputUnaryOp nor :67-86 sets it)
            return
        if not isinstance(op1, RefCt):
            level = min(op0.Level(), opOut.Level())
            opOut.Resize(op0.Degree(), level)
            op1 = self._pt(op1, level, op0, op0.Scale)
            self.evaluateInPlace(level, op0, op1, opOut, sub)
            return
        degree = max(op0.Degree(), op1.Degree(), opOut.Degree())
        level = min(op0.Level(), op1.Level(), opOut.Level())
        opOut.Resize(degree, level)
        self.evaluateInPlace(level, op0, op1, opOut, sub)
        if sub and op0.Degree() < op1.Degree():  # :152-156
            for i in range(op0.Degree() + 1, op1.Degree() + 1):
                opOut.Value[i] = self._r(level).unop("Neg", opOut.Value[i])

    def Add(self, op0, op1, opOut):
        self._addsub(op0, op1, opOut, False)

    def Sub(self, op0, op1, opOut):
        self._addsub(op0, op1, opOut, True)

    def evaluateInPlace(self, level, c0, c1, opOut, sub):
        """:221-408, branch by branch; self.branch records which of the nine was taken"""
        r = self._r(level)
        cut = lambda ct: RefCt([v[: level + 1] for v in ct.Value], ct.Scale, ct.LogSlots)
        maxD, minD = max(c0.Degree(), c1.Degree()), min(c0.Degree(), c1.Degree())
        c0Scale, c1Scale = Scale(c0.Scale), Scale(c1.Scale)
        cmp = c0Scale.Cmp(c1Scale)
        tmp0 = tmp1 = None

        def mul_into(src, n, dst):  # eval.Mul(src, ratioInt, dst) (:629-666 with an integer)
            self.Mul(src, n, dst)

        where = "op0" if opOut is c0 else ("op1" if opOut is c1 else "new")
        self.branch = (where, cmp)
        if opOut is c0:
            if cmp == 1:
                ratioInt = c0Scale.Div(c1Scale).Int()
                if ratioInt > 0:
                    tmp1 = self.NewCiphertext(c1.Degree(), level)
                    mul_into(cut(c1), ratioInt, tmp1)
            elif cmp == -1:
                ratioInt = c1Scale.Div(c0Scale).Int()
                if ratioInt > 0:
                    mul_into(c0, ratioInt, c0)
                    opOut.Scale = Scale(c1.Scale)
                    tmp1 = cut(c1)
            else:
                tmp1 = cut(c1)
            tmp0 = c0
        elif opOut is c1:
            if cmp == 1:
                ratioInt = c0Scale.Div(c1Scale).Int()
                if ratioInt > 0:
                    mul_into(c1, ratioInt, opOut)
                    opOut.Scale = Scale(c0.Scale)
                    tmp0 = cut(c0)
            elif cmp == -1:
                ratioInt = c1Scale.Div(c0Scale).Int()
                if ratioInt > 0:
                    tmp0 = self.NewCiphertext(c0.Degree(), level)
                    mul_into(cut(c0), ratioInt, tmp0)
            else:
                tmp0 = cut(c0)
            tmp1 = c1
        else:
            if cmp == 1:
                ratioInt = c0Scale.Div(c1Scale).Int()
                if ratioInt > 0:
                    tmp1 = self.NewCiphertext(c1.Degree(), level)
                    mul_into(cut(c1), ratioInt, tmp1)
                    tmp0 = cut(c0)
            elif cmp == -1:
                ratioInt = c1Scale.Div(c0Scale).Int()
                if ratioInt > 0:
                    tmp0 = self.NewCiphertext(c0.Degree(), level)
                    mul_into(cut(c0), ratioInt, tmp0)
                    tmp1 = cut(c1)
            else:
                tmp0, tmp1 = cut(c0), cut(c1)
        for i in range(minD + 1):  # :390-392
            opOut.Value[i] = r.binop("Sub" if sub else "Add", tmp0.Value[i][: level + 1], tmp1.Value[i][: level + 1])
        opOut.Scale = c0Scale.Max(c1Scale)  # :394
        if c0.Degree() > c1.Degree() and tmp0 is not opOut:  # :399-407
            for i in range(minD + 1, maxD + 1):
                opOut.Value[i] = tmp0.Value[i][: level + 1].copy()
        elif c1.Degree() > c0.Degree() and tmp1 is not opOut:
            for i in range(minD + 1, maxD + 1):
                opOut.Value[i] = tmp1.Value[i][: level + 1].copy()

    # -- Mul / MulRelin (:613-872)
    def Mul(self, op0, op1, opOut, relin=False):
        if self._is_scalar(op1):
            level = min(op0.Level(), opOut.Level())
            opOut.Resize(op0.Degree(), level)
            scale = Scale(1) if self._is_int(op1) else Scale(self.Q[level])
            s0, s1 = self._rns(level, scale, op1)
            r = self._r(level)
            new = op0.Scale.Mul(scale)
            opOut.Value = [r.MulDoubleRNSScalar(v[: level + 1], s0, s1) for v in op0.Value]
            opOut.Scale = new
            return
        if not isinstance(op1, RefCt):
            level = min(op0.Level(), opOut.Level())
            opOut.Resize(op0.Degree(), level)
            op1 = self._pt(op1, level, op0, Scale(self.Q[level]))  # :681-694
        self.mulRelin(op0, op1, relin, opOut)

    def MulRelin(self, op0, op1, opOut):
        self.Mul(op0, op1, opOut, True)

    def mulRelin(self, op0, op1, relin, opOut):
        level = min(op0.Level(), op1.Level(), opOut.Level())
        r = self._r(level)
        scale = op0.Scale.Mul(op1.Scale)
        if op0.Degree() == 1 and op1.Degree() == 1:
            a = np.stack([v[: level + 1] for v in op0.Value])
            b = np.stack([v[: level + 1] for v in op1.Value])
            out = self.oev.CKKSMulRelin(a, b, self.rlk if relin else None, relin)  # :780-839 (pinned by the oracle's own tests)
            opOut.Value = [np.array(v[: level + 1]) for v in out]
        else:
            pt, ct = (op0, op1) if op0.Degree() == 0 else (op1, op0)
            c00 = r.unop("MForm", pt.Value[0][: level + 1])
            opOut.Value = [r.binop("MulCoeffsMontgomery", c00, v[: level + 1]) for v in ct.Value]
        opOut.Scale = scale

    # -- MulThenAdd / MulRelinThenAdd (:909-1173)
    def MulThenAdd(self, op0, op1, opOut, relin=False):
        if isinstance(op1, RefCt):
            if op0 is opOut or op1 is opOut:
                raise ValueError("cannot MulThenAdd: opOut must be different from op0 and op1")
            level = min(op0.Level(), op1.Level(), opOut.Level())
            opOut.Resize(opOut.Degree(), level)
            return self.mulRelinThenAdd(op0, op1, relin, opOut)
        level = min(op0.Level(), opOut.Level())
        opOut.Resize(op0.Degree(), opOut.Level())
        vector = not self._is_scalar(op1)
        cmp = op0.Scale.Cmp(opOut.Scale)
        if cmp == 0:
            if not vector and self._is_int(op1):
                scale = Scale(1)
            else:
                scale = Scale(self.Q[level])
                self.Mul(opOut, scale.Int(), opOut)  # at opOut's own level (:959-964, :999-1003)
                opOut.Scale = opOut.Scale.Mul(scale)
        elif cmp == -1:
            scale = opOut.Scale.Div(op0.Scale)
        else:
            raise ValueError("cannot MulThenAdd: op0.Scale > opOut.Scale is not supported")
        if vector:
            return self.MulThenAdd(op0, self._pt(op1, level, op0, scale), opOut)
        s0, s1 = self._rns(level, scale, op1)
        r = self._r(level)
        for i in range(op0.Degree() + 1):
            head = r.MulDoubleRNSScalarThenAdd(op0.Value[i][: level + 1], s0, s1, opOut.Value[i][: level + 1])
            opOut.Value[i] = np.concatenate([head, opOut.Value[i][level + 1:]])

    def MulRelinThenAdd(self, op0, op1, opOut):
        self.MulThenAdd(op0, op1, opOut, True)

    def mulRelinThenAdd(self, op0, op1, relin, opOut):
        level = opOut.Level()
        resScale = op0.Scale.Mul(op1.Scale)
        if opOut.Scale.Cmp(resScale) == -1:
            ratio = resScale.Div(opOut.Scale)
            if ratio.Float64() >= 2.0:
                self.Mul(opOut, ratio.fraction(), opOut)  # a *big.Float operand (:1091)
                opOut.Scale = resScale
        if op0.Degree() == 1 and op1.Degree() == 1:
            acc = list(opOut.Value) + ([np.zeros_like(opOut.Value[0])] if opOut.Degree() < 2 else [])
            out = ckks_mul_relin_then_add(self.ringQ, level, op0.Value, op1.Value, acc, None, self.oev if relin else None,
                                          self.rlk if relin else None)
            opOut.Value = out + (opOut.Value[2:] if relin else [])
        else:
            opOut.Resize(max(op0.Degree(), opOut.Degree()), level)
            n = op0.Degree() + 1
            opOut.Value[:n] = ckks_mul_pt(self.ringQ, level, op0.Value, op1.Value[0], opOut.Value[:n])

    # -- Relinearize, Rescale, RescaleTo, SetScale, Rotate
    def Relinearize(self, op0, opOut):
        level = min(op0.Level(), opOut.Level())
        out = self.oev.Relinearize(np.stack([v[: level + 1] for v in op0.Value]), self.rlk)
        opOut.Value, opOut.Scale, opOut.LogSlots = [np.array(v) for v in out], Scale(op0.Scale), op0.LogSlots

    def Rescale(self, op0, opOut):
        self.RescaleTo(op0, None, opOut)

    def RescaleTo(self, op0, minScale, opOut):
        level = op0.Level()
        if level == 0:
            raise ValueError("cannot Rescale: input Ciphertext already at level 0")
        scale, nb = Scale(op0.Scale), 0
        if minScale is None:  # Rescale (:477-521): once
            scale, nb = scale.Div(self.Q[level]), 1
        else:
            floor, new = Scale(minScale).Div(2), level
            while new >= 0:
                s = scale.Div(self.Q[new])
                if s.Cmp(floor) == -1:
                    break
                scale, nb, new = s, nb + 1, new - 1
        vals = [self._r(level).DivRoundByLastModulusManyNTT(nb, v[: level + 1]) if nb else v[: level + 1].copy() for v in op0.Value]
        opOut.Value, opOut.Scale, opOut.LogSlots = [v[: level + 1 - nb] for v in vals], scale, op0.LogSlots

    def SetScale(self, ct, scale):
        scale = Scale(scale)
        self.Mul(ct, scale.Div(ct.Scale).fraction(), ct)
        self.RescaleTo(ct, scale, ct)
        ct.Scale = scale

    def Rotate(self, op0, k, opOut):
        g = pow(5, k & (2 * self.ringQ.N - 1), 2 * self.ringQ.N)
        level = min(op0.Level(), opOut.Level())
        out = self.oev.Automorphism(np.stack([v[: level + 1] for v in op0.Value]), g, self.gks[g])
        opOut.Value, opOut.Scale, opOut.LogSlots = [np.array(v) for v in out], Scale(op0.Scale), op0.LogSlots


class _MoreMethods:
    """the key-switching methods (:1183-1318) and the small ones, over the oracle's evaluator"""

    def _auto(self, op0, g, opOut):
        level = min(op0.Level(), opOut.Level())
        out = self.oev.Automorphism(np.stack([v[: level + 1] for v in op0.Value]), g, self.gks[g])
        opOut.Value, opOut.Scale, opOut.LogSlots = [np.array(v) for v in out], Scale(op0.Scale), op0.LogSlots

    def Conjugate(self, op0, opOut):
        self._auto(op0, 2 * self.ringQ.N - 1, opOut)  # GaloisElementOrderTwoOrthogonalSubgroup

    def RotateHoisted(self, ctIn, rotations, opOut: dict):
        level, levelP = ctIn.Level(), self.oev.ringP.MaxLevel()
        ct = np.stack([v[: level + 1] for v in ctIn.Value])
        dq, dp = self.oev.DecomposeNTT(level, levelP, levelP + 1, ct[1])  # :1248
        for k in rotations:
            g = pow(5, k & (2 * self.ringQ.N - 1), 2 * self.ringQ.N)
            out = self.oev.AutomorphismHoisted(ct, dq, dp, g, self.gks[g])  # :1250
            opOut[k].Value, opOut[k].Scale, opOut[k].LogSlots = [np.array(v) for v in out], Scale(ctIn.Scale), ctIn.LogSlots

    def InnerSum(self, ctIn, batchSize, n, opOut):
        from oracle import circuits as OC
        level = min(ctIn.Level(), opOut.Level())
        out = OC.InnerSumEvaluator(self.oev, self.gks).PartialTracesSum(np.stack([v[: level + 1] for v in ctIn.Value]), batchSize, n)  # :1298
        opOut.Value, opOut.Scale, opOut.LogSlots = [np.array(v) for v in out], Scale(ctIn.Scale), ctIn.LogSlots

    RotateAndAdd = InnerSum  # :1315-1318: the same PartialTracesSum without the checks on n * batchSize

    def ApplyEvaluationKey(self, op0, evk, opOut):
        """core/rlwe/evaluator_evaluationkey.go:36-106, equal ring degrees: GadgetProduct of c1, c0 added"""
        level = min(op0.Level(), opOut.Level())
        t = self.oev.GadgetProduct(level, op0.Value[1][: level + 1], evk)
        opOut.Value = [self._r(level).binop("Add", op0.Value[0][: level + 1], t[0][: level + 1]), np.array(t[1][: level + 1])]
        opOut.Scale, opOut.LogSlots = Scale(op0.Scale), op0.LogSlots

    def ScaleUp(self, op0, scale, opOut):  # :433-443
        new = op0.Scale.Mul(scale)
        self.Mul(op0, min(Scale(scale).Int(), (1 << 64) - 1), opOut)
        opOut.Scale = new

    def DropLevel(self, op0, levels):  # :467-469
        op0.Resize(op0.Degree(), op0.Level() - levels)


for _name, _f in vars(_MoreMethods).items():
    if not _name.startswith("__"):
        setattr(RefEvaluator, _name, _f)
