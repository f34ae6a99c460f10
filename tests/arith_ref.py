"""Exact references and operand sets for the device arithmetic primitives (he_debug_arith, include/hering_debug.h): host only.

Every kernel of csrc/kernels.hip is built on about twenty scalar primitives (csrc/modarith.h and the butterflies / double-precision
helpers of kernels.hip), each with a written exactness argument on a domain.  This module holds, for each of them,

* the truth, in Python integers: the residue class (r 2^64 = x y mod q ...), the stated range, and -- where the reference's lazy
  WORD is visible through the API -- the word of the oracle (O.MRedLazy, O.BRedLazy, O.BRedAddLazy, O.MFormLazy, O.IMForm, taken
  through the oracle's vector forms of the same functions);
* the expected device word as a fast vector restatement (numpy), which tests/test_arith_host.py holds against that truth on every
  operand set, so that tests/test_gpu_arith.py compares the device with one array per set;
* a numpy restatement of the two 32-bit-word Montgomery schedules (the C++ form of modarith.h and the column form of the
  hand-written sequence) that asserts the written argument itself: no 64-bit accumulator overflows, and that counts the four carry
  points of the column form;
* a bit-exact model of the double-precision family built from integers with an explicit round-to-nearest-even helper;
* the operand sets: per op and per modulus, families "lattice", "zero" (m = 0 rounds and the documented exception of
  mred_lazy_w32), "top" (the top of the op's domain), "hunt" (low words next to 2^32, for the carries), "keys" (mred_lazy_w32
  only: a second operand at or above q), "half" (double precision: quotients next to a half-integer / an integer) and "random"
  (2^16 uniform tuples).  Every tuple is clipped to the op's domain and the generators assert that.

Domains (where each comes from is in NOTES.md, "The arithmetic primitives"):
  B(q) = 4q for q >= 2^58 (the Harvey butterflies keep [0, 4q)), 34q for q < 2^58 (the correction-free forward transform:
  17 stages of + 2q); the double-precision products take |a| <= 36q (a lazy input word below 2q plus 34q, kernels.hip
  "34q + input") for the magnitude claim and |a| < 2^53 for exactness."""
from __future__ import annotations

import functools
import itertools

import numpy as np

from oracle import oracle as O
from tests import boundary as Bd
from tests.conftest import Qi60
from tests.helpers import rng_for

LOGN = 10
N = 1 << LOGN
M64 = (1 << 64) - 1
R = 1 << 64
U = np.uint64
N_RANDOM = 1 << 16
MAX_SET = 1 << 17

OPS = ["MRED_LAZY", "MRED", "MRED_LAZY_W32", "MRED_LAZY_ASM", "MRED128_LAZY", "BRED_ADD_LAZY", "BRED_ADD", "BRED_LAZY", "BRED",
       "MFORM_LAZY", "MFORM", "IMFORM_LAZY", "IMFORM", "BFLY_FWD", "BFLY_FWD_ASM", "BFLY_FWD_NC", "BFLY_FWD_NC_ASM", "BFLY_INV",
       "BFLY_INV_ASM", "BFLY_INV_SCALED", "BFLY_INV_SCALED_ASM", "MODMUL_F64", "REDUCE_F64", "CANON_F64D", "CANON_F64", "U52_TO_F64",
       "F64_TO_U52", "HALVE", "AUTO_DEST"]
OP_ID = {name: i for i, name in enumerate(OPS)}  # HE_ARITH_* of include/hering_debug.h
F64_OPS = ("MODMUL_F64", "REDUCE_F64", "CANON_F64D", "CANON_F64", "U52_TO_F64", "F64_TO_U52")
NC_OPS = ("BFLY_FWD_NC", "BFLY_FWD_NC_ASM")
PAIR_OPS = tuple(o for o in OPS if o.startswith("BFLY_"))


# ---------------------------------------------------------------------------------------------------------------
# moduli: one N = 2^10 ring per arithmetic class
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def moduli():
    """[(name, q, ring index, limb)]: the class edges, the 32-bit edge (q >> 32 is 1 or 0) and the 27-bit prime of rgsw_edges"""
    from tests import rgsw_edges as E
    lr = LOGN + 1
    named = [("top61", Bd.primes_below(61, lr, 1)[0]), ("qi60_0", Qi60[0]), ("min58", Bd.primes_above(58, lr, 1)[0]),
             ("max58", Bd.primes_below(58, lr, 1)[0]), ("min47", Bd.primes_above(47, lr, 1)[0]),
             ("max47", Bd.primes_below(47, lr, 1)[0]), ("min32", Bd.primes_above(32, lr, 1)[0]),
             ("max32", Bd.primes_below(32, lr, 1)[0]), ("q27", E.moduli(LOGN, (27,))[0][0])]
    out, count, seen = [], [0, 0, 0], set()
    for name, q in named:
        assert q % (2 * N) == 1 and O.IsPrime(q), name
        if q in seen:
            continue
        seen.add(q)
        c = Bd.modulus_class(q)
        out.append((name, q, c, count[c]))
        count[c] += 1
    assert [c for _, _, c, _ in out] == sorted((c for _, _, c, _ in out), reverse=True)  # largest first, by class
    return out


def ring_moduli(c):
    return [q for _, q, cc, _ in moduli() if cc == c]


def applies(op, q):
    """does the op exist at this modulus: the double-precision family below 2^47, the correction-free butterfly below 2^58"""
    if op in F64_OPS:
        return q < (1 << Bd.CLASS_BITS[0])
    if op in NC_OPS:
        return q < (1 << Bd.CLASS_BITS[1])
    return op != "AUTO_DEST"


def cases():
    return [(op, name) for op in OPS for name, q, _, _ in moduli() if applies(op, q)]


def lazy_bound(q):
    """B(q): what a butterfly hands its Montgomery product"""
    return 4 * q if q >= (1 << Bd.CLASS_BITS[1]) else 34 * q


class Consts:
    """the constants of csrc/modarith.h's ModConst, from Python integers"""

    def __init__(self, q):
        self.q = q
        self.qinv = pow(q, -1, R)
        brc = (1 << 128) // q
        self.brc0, self.brc1 = brc >> 64, brc & M64
        self.ninv = pow(N, -1, q) * R % q  # MForm(N^-1)
        self.rinv = pow(R, -1, q)
        self.rq_m, self.rq_e = rn_ratio(1, q)  # 1 / q as a double: rq_m 2^rq_e


@functools.lru_cache(None)
def consts(q):
    return Consts(q)


# ---------------------------------------------------------------------------------------------------------------
# round to nearest even, from integers
# ---------------------------------------------------------------------------------------------------------------
def rne_shift(i, s):
    """i / 2^s rounded to the nearest integer, ties to even (s <= 0: exact)"""
    if s <= 0:
        return i << -s
    fl, rem, half = i >> s, i & ((1 << s) - 1), 1 << (s - 1)  # floor and a non-negative remainder, for negative i too
    return fl + 1 if rem > half or (rem == half and (fl & 1)) else fl


def rn(i, e=0):
    """the double nearest to i 2^e as (m, e') with |m| <= 2^53 (no subnormals or overflow at these magnitudes)"""
    s = abs(i).bit_length() - 53
    return (i, e) if s <= 0 else (rne_shift(i, s), e + s)


def rn_int(i):
    """the double nearest to the integer i, as an integer"""
    m, e = rn(i)
    return m << e


def rn_ratio(num, den):
    """the double nearest to num / den (positive): 55 quotient bits and a sticky bit, then one rounding"""
    k = 55 + den.bit_length() - num.bit_length() + 1
    qt, rem = divmod(num << k, den)
    return rn(2 * qt + (1 if rem else 0), -k - 1)


def to_int_rne(m, e):
    return rne_shift(m, -e)  # rint


def to_int_floor(m, e):
    return m << e if e >= 0 else m >> -e


def is_double(i):
    return rn_int(i) == i


def modmul_f64_model(a, w, q):
    """kernels.hip modmul_f64 from integers: h = rn(a w), l = a w - h, c = rint(rn(h rq)), r = rn(rn(h - c q) + l)"""
    k = consts(q)
    p = a * w
    h = rn_int(p)
    l = p - h
    assert is_double(l)  # the error of a product is a double (fma(a, w, -h) is exact)
    c = to_int_rne(*rn(h * k.rq_m, k.rq_e))
    return rn_int(rn_int(h - c * q) + l)


def reduce_f64_model(x, q):
    k = consts(q)
    return rn_int(x - to_int_rne(*rn(x * k.rq_m, k.rq_e)) * q)


def canon_f64d_model(x, q):
    k = consts(q)
    t = rn_int(x - to_int_floor(*rn(x * k.rq_m, k.rq_e)) * q)
    if t < 0:
        t = rn_int(t + q)
    if t >= q:
        t = rn_int(t - q)
    return t


def f64_bits(vals):
    """bit patterns of integer-valued doubles (every zero of these ops is +0: an exact cancellation in round-to-nearest, and no
    input is -0)"""
    vals = list(vals)
    f = np.array([float(v) for v in vals], dtype=np.float64)
    assert all(int(x) == v for x, v in zip(f.tolist(), vals)), "a model value is not a double"
    return f.view(np.uint64).copy()


def bits_f64_int(words):
    f = np.ascontiguousarray(words, dtype=np.uint64).view(np.float64)
    return [int(v) for v in f.tolist()]


# ---------------------------------------------------------------------------------------------------------------
# the two word-serial Montgomery schedules, restated (numpy uint64, every addition checked)
# ---------------------------------------------------------------------------------------------------------------
_M32, _S32 = U(0xFFFFFFFF), U(32)


def _add(a, b, what):
    s = a + b
    assert not (s < a).any(), f"64-bit accumulator overflow: {what}"
    return s


def _addc(a, b):
    s = a + b
    return s, (s < a)


def w32_schedule(x, y, q):
    """modarith.h mred_lazy_w32, statement by statement; asserts the bounds of its comment (u, v, a, b and the result fit)"""
    x, y = np.asarray(x, dtype=U), np.asarray(y, dtype=U)
    q0, q1, nq = U(q & 0xFFFFFFFF), U(q >> 32), U((-consts(q).qinv) & 0xFFFFFFFF)
    x0, x1, y0, y1 = x & _M32, x >> _S32, y & _M32, y >> _S32
    t = x0 * y0
    u = _add(x1 * y0, t >> _S32, "u")
    m = ((t & _M32) * nq) & _M32
    c = _add(m * q0, t & _M32, "c")
    assert not (c & _M32).any()
    v = _add(_add(m * q1, u, "v"), c >> _S32, "v")
    a = _add(x0 * y1, v & _M32, "a")
    b = _add(_add(x1 * y1, a >> _S32, "b"), v >> _S32, "b")
    m = ((a & _M32) * nq) & _M32
    c = _add(m * q0, a & _M32, "c'")
    assert not (c & _M32).any()
    return _add(_add(m * q1, b, "r"), c >> _S32, "r")


def column_schedule(x, w, q):
    """kernels.hip mred_lazy_col_asm, instruction by instruction: three 64-bit accumulators L, M, H.  Returns (r, carries) with
    carries[k] the carry-out taken by the k-th v_addc; asserts that no other addition overflows (the middle column above all)."""
    x, w = np.asarray(x, dtype=U), np.asarray(w, dtype=U)
    q0, q1, nq = U(q & 0xFFFFFFFF), U(q >> 32), U((-consts(q).qinv) & 0xFFFFFFFF)
    x0, x1, w0, w1 = x & _M32, x >> _S32, w & _M32, w >> _S32
    L, M, H = x0 * w0, x0 * w1, x1 * w1
    M = _add(M, x1 * w0, "M = x0 w1 + x1 w0")
    m = ((L & _M32) * nq) & _M32
    L, c1 = _addc(L, m * q0)
    assert not (L & _M32).any()
    M = _add(M, c1.astype(U) << _S32, "M.hi + carry")
    M = _add(M, m * q1, "M += m q1")
    lo = (M & _M32) + (L >> _S32)
    c2 = (lo >> _S32) != 0
    M = _add((M & ~_M32) | (lo & _M32), c2.astype(U) << _S32, "M.hi + carry of L.hi")
    m = ((M & _M32) * nq) & _M32
    M, c3 = _addc(M, m * q0)
    assert not (M & _M32).any()
    H = _add(H, c3.astype(U) << _S32, "H.hi + carry")
    lo = (H & _M32) + (M >> _S32)
    c4 = (lo >> _S32) != 0
    H = _add((H & ~_M32) | (lo & _M32), c4.astype(U) << _S32, "H.hi + carry of M.hi")
    return _add(H, m * q1, "r = H + m q1"), (c1, c2, c3, c4)


def carries_reachable(q, bound):
    """Which of the four carries CAN be one for x < bound, w < q, by interval arithmetic on the schedule: the third needs
    M + m q0 >= 2^64 and the fourth H.lo + M.hi >= 2^32, which a modulus just above a power of two (q0 a few thousand) or an
    operand of few high bits cannot reach.  Where a carry is reachable the sets must show both of its values; where it is not,
    the sets must show it zero throughout."""
    m32 = (1 << 32) - 1
    x0, x1, w0, w1, q0, q1 = min(bound - 1, m32), (bound - 1) >> 32, min(q - 1, m32), (q - 1) >> 32, q & m32, q >> 32
    m_max = min(M64, x0 * w1 + x1 * w0 + (1 << 32) + m32 * q1 + m32 + (1 << 32))  # M before the second round
    c3 = m_max + m32 * q0 >= R
    m_hi = min(M64, m_max + m32 * q0) >> 32
    h_lo = min(m32, x1 * w1 + (1 << 32))
    return (True, True, c3, h_lo + m_hi > m32)


# ---------------------------------------------------------------------------------------------------------------
# expected device words (vector) and the truth they are held against (Python integers)
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _oracle_ring(q):
    return O.Ring(N, [q])


def _oracle(q, kind, name, x, y=None):
    """the oracle's vector form of a scalar helper (MulCoeffsMontgomeryLazy = MRedLazy per word, ...) over any number of words"""
    ring, n = _oracle_ring(q), len(x)
    pad = (-n) % N
    xs = np.concatenate([x, np.zeros(pad, dtype=U)]).reshape(-1, 1, N)
    ys = None if y is None else np.concatenate([y, np.zeros(pad, dtype=U)]).reshape(-1, 1, N)
    out = [ring.binop(name, xs[k], ys[k]) if kind == "bin" else ring.unop(name, xs[k]) for k in range(len(xs))]
    return np.concatenate(out).reshape(-1)[:n]


def _cred(r, q):
    return np.where(r >= U(q), r - U(q), r)


def mred_lazy_word(x, y, q):
    return _oracle(q, "bin", "MulCoeffsMontgomeryLazy", x, y)


def w32_word(x, y, q):
    """the mred_lazy word, minus q where the low 64 bits of x y are zero (the exception modarith.h states)"""
    r = mred_lazy_word(x, y, q)
    return np.where(x * y == U(0), r - U(q), r)  # (uint64 products wrap: exactly the low 64 bits)


def expected(op, q, args):
    """(out0, out1 or None) of he_debug_arith(op) at modulus q: uint64 arrays"""
    k, uq, twoq = consts(q), U(q), U(2 * q)
    a = args[0]
    b = args[1] if len(args) > 1 else None
    c = args[2] if len(args) > 2 else None
    if op == "MRED_LAZY":
        return mred_lazy_word(a, b, q), None
    if op == "MRED":
        return _oracle(q, "bin", "MulCoeffsMontgomery", a, b), None
    if op in ("MRED_LAZY_W32", "MRED_LAZY_ASM"):
        return w32_word(a, b, q), None
    if op == "MRED128_LAZY":  # hi - mulhi(lo qinv, q) + q: hi plus the MRedLazy word of (lo, 1), whose high product word is zero
        return a + mred_lazy_word(b, np.ones_like(b), q), None
    if op == "BRED_ADD_LAZY":
        return _oracle(q, "un", "ReduceLazy", a), None
    if op == "BRED_ADD":
        return _oracle(q, "un", "Reduce", a), None
    if op == "BRED_LAZY":
        return _oracle(q, "bin", "MulCoeffsBarrettLazy", a, b), None
    if op == "BRED":
        return _oracle(q, "bin", "MulCoeffsBarrett", a, b), None
    if op == "MFORM_LAZY":
        return _oracle(q, "un", "MFormLazy", a), None
    if op == "MFORM":
        return _oracle(q, "un", "MForm", a), None
    if op == "IMFORM_LAZY":  # q - mulhi(a qinv, q): the MRedLazy word of (a, 1), whose high product word is zero
        return mred_lazy_word(a, np.ones_like(a), q), None
    if op == "IMFORM":
        return _oracle(q, "un", "IMForm", a), None
    if op in ("BFLY_FWD", "BFLY_FWD_ASM"):
        u, v = np.where(a >= twoq, a - twoq, a), w32_word(b, c, q)
        return u + v, u + twoq - v
    if op in NC_OPS:
        r = w32_word(b, c, q)
        return a + r, a + twoq - r
    if op in ("BFLY_INV", "BFLY_INV_ASM"):
        x = a + b
        d = a + twoq - b
        return np.where(x >= twoq, x - twoq, x), (mred_lazy_word if op == "BFLY_INV" else w32_word)(d, c, q)
    if op in ("BFLY_INV_SCALED", "BFLY_INV_SCALED_ASM"):
        x = a + b
        if op.endswith("ASM"):
            x = np.where(x >= twoq, x - twoq, x)
        ninv = np.full_like(a, k.ninv)
        return _cred(w32_word(x, ninv, q), q), _cred(w32_word(a + twoq - b, c, q), q)
    if op == "HALVE":
        return np.where((a & U(1)) != 0, (a + uq) >> U(1), a >> U(1)), None
    if op == "MODMUL_F64":
        return f64_bits(modmul_f64_model(x, w, q) for x, w in zip(bits_f64_int(a), bits_f64_int(b))), None
    if op == "REDUCE_F64":
        return f64_bits(reduce_f64_model(x, q) for x in bits_f64_int(a)), None
    if op == "CANON_F64D":
        return f64_bits(canon_f64d_model(x, q) for x in bits_f64_int(a)), None
    if op == "CANON_F64":
        return np.array([canon_f64d_model(x, q) for x in bits_f64_int(a)], dtype=U), None
    if op == "U52_TO_F64":
        return f64_bits(a.tolist()), None
    if op == "F64_TO_U52":
        return np.array(bits_f64_int(a), dtype=U), None
    raise ValueError(op)


def check_truth(op, q, args, out0, out1, magnitude=None):
    """the claims of the primitive, in Python integers, on every tuple: residue class, stated range; (out0, out1) are the
    expected words.  Raises AssertionError naming the first tuple that misses."""
    k = consts(q)
    A = [x.tolist() for x in args]
    o0 = out0.tolist()
    o1 = out1.tolist() if out1 is not None else None
    n, rinv, ninv = len(o0), k.rinv, k.ninv

    def fail(i, what):
        raise AssertionError(f"{op} mod {q:#x}: {what} at tuple {i}: " + " ".join(f"{x[i]:#x}" for x in A) + f" -> {o0[i]:#x}"
                             + (f" {o1[i]:#x}" if o1 else ""))

    def every(ok, what):
        for i in range(n):
            if not ok(i):
                fail(i, what)

    if op in ("MRED_LAZY", "MRED", "MRED_LAZY_W32", "MRED_LAZY_ASM"):
        x, y = A
        every(lambda i: (o0[i] * R - x[i] * y[i]) % q == 0, "r 2^64 != x y mod q")
        every(lambda i: o0[i] < (q if op == "MRED" else 2 * q), "range")
        if op in ("MRED_LAZY_W32", "MRED_LAZY_ASM"):  # = (x y + M q) / 2^64 with M = -x y q^-1 mod 2^64, the integer itself
            every(lambda i: o0[i] * R == x[i] * y[i] + ((-x[i] * y[i] * k.qinv) % R) * q, "not (T + M q) / 2^64")
    elif op == "MRED128_LAZY":
        hi, lo = A
        every(lambda i: (o0[i] * R - (hi[i] * R + lo[i])) % q == 0 and o0[i] < 2 * q, "class or range")
    elif op in ("BRED_ADD_LAZY", "BRED_ADD"):
        every(lambda i: (o0[i] - A[0][i]) % q == 0 and o0[i] < (q if op == "BRED_ADD" else 2 * q), "class or range")
    elif op in ("BRED_LAZY", "BRED"):
        every(lambda i: (o0[i] - A[0][i] * A[1][i]) % q == 0 and o0[i] < (q if op == "BRED" else 2 * q), "class or range")
    elif op in ("MFORM_LAZY", "MFORM"):
        every(lambda i: (o0[i] - A[0][i] * R) % q == 0 and o0[i] < (q if op == "MFORM" else 2 * q), "class or range")
    elif op in ("IMFORM_LAZY", "IMFORM"):
        every(lambda i: (o0[i] * R - A[0][i]) % q == 0 and (o0[i] < q if op == "IMFORM" else 0 < o0[i] <= q), "class or range")
    elif op == "HALVE":
        every(lambda i: (2 * o0[i] - A[0][i]) % q == 0 and o0[i] < q, "class or range")
    elif op in ("BFLY_FWD", "BFLY_FWD_ASM"):
        a, b, w = A
        every(lambda i: (o0[i] - (a[i] + b[i] * w[i] * rinv)) % q == 0 and (o1[i] - (a[i] - b[i] * w[i] * rinv)) % q == 0, "class")
        every(lambda i: o0[i] < 4 * q and o1[i] < 4 * q, "[0, 4q)^2 -> [0, 4q)^2")
    elif op in NC_OPS:
        a, b, w = A
        every(lambda i: (o0[i] - (a[i] + b[i] * w[i] * rinv)) % q == 0 and (o1[i] - (a[i] - b[i] * w[i] * rinv)) % q == 0, "class")
        every(lambda i: o0[i] < a[i] + 2 * q and 0 < o1[i] <= a[i] + 2 * q and a[i] + 2 * q <= 34 * q, "output below input + 2q <= 34q")
    elif op in ("BFLY_INV", "BFLY_INV_ASM"):
        a, b, w = A
        every(lambda i: (o0[i] - (a[i] + b[i])) % q == 0 and (o1[i] * R - (a[i] - b[i]) * w[i]) % q == 0, "class")
        every(lambda i: o0[i] < 2 * q and o1[i] < 2 * q, "[0, 2q)^2 -> [0, 2q)^2")
    elif op in ("BFLY_INV_SCALED", "BFLY_INV_SCALED_ASM"):
        a, b, w = A
        every(lambda i: (o0[i] * R - (a[i] + b[i]) * ninv) % q == 0 and (o1[i] * R - (a[i] - b[i]) * w[i]) % q == 0, "class")
        every(lambda i: o0[i] < q and o1[i] < q, "canonical outputs")
    elif op == "MODMUL_F64":
        a, w, r = bits_f64_int(args[0]), bits_f64_int(args[1]), bits_f64_int(out0)
        A[:] = [a, w]
        every(lambda i: (r[i] - a[i] * w[i]) % q == 0, "r != a w mod q")
        if magnitude is not None:
            every(lambda i: abs(a[i]) > magnitude or abs(r[i]) < 2 * q, "|r| < 2q")
    elif op in ("REDUCE_F64", "CANON_F64D", "CANON_F64"):
        x = bits_f64_int(args[0])
        r = o0 if op == "CANON_F64" else bits_f64_int(out0)
        A[:] = [x]
        every(lambda i: (r[i] - x[i]) % q == 0 and (abs(r[i]) < q if op == "REDUCE_F64" else 0 <= r[i] < q), "class or range")
    elif op == "U52_TO_F64":
        every(lambda i: bits_f64_int(out0[i:i + 1])[0] == A[0][i], "value")
    elif op == "F64_TO_U52":
        every(lambda i: bits_f64_int(args[0][i:i + 1])[0] == o0[i], "value")
    else:
        raise ValueError(op)


# ---------------------------------------------------------------------------------------------------------------
# operand sets
# ---------------------------------------------------------------------------------------------------------------
def _arr(vals):
    return np.array([int(v) for v in vals], dtype=U)


def edge_values(q, bound):
    """the lattice's values below `bound`"""
    top = (bound - 1) >> 32 << 32  # the largest word of the domain whose low 32 bits are all zero
    vals = [0, 1, 2, q - 2, q - 1, q, q + 1, 2 * q - 1, 2 * q, 4 * q - 1, bound - 1, bound - 2, top, top - (1 << 32), top - 1,
            (bound - 1) | 0xFFFFFFFF if ((bound - 1) | 0xFFFFFFFF) < bound else top - 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1]
    out = sorted({v for v in vals if 0 <= v < bound})
    assert out and out[-1] == bound - 1
    return out


def _ri(rng, lo, hi):
    """one integer in [lo, hi), any size (the bias of the modulo is below 2^-32)"""
    return lo + int.from_bytes(rng.bytes(12), "little") % (hi - lo)


def _uniform(rng, bound, n):
    """n uniform words below `bound` <= 2^64"""
    if bound >= R:
        return Bd.wild_words(rng, n)
    return rng.integers(0, bound, size=n, dtype=np.uint64)


def _lattice(bounds, q):
    cols = list(zip(*itertools.product(*[edge_values(q, b) for b in bounds])))
    return tuple(_arr(c) for c in cols)


def _zero_pairs(rng, q, bx, by, n=256):
    """(x, y), x < bx, y < by, whose product has its low 32 bits zero (an m = 0 first round) -- and, second half, its low 64 bits
    zero (both rounds; the exception of mred_lazy_w32): x = u 2^a, y = v 2^(64 - a) where the domain has such words, and a zero
    operand everywhere"""
    xs, ys, kinds = [], [], []
    for _ in range(n):
        if bx > (1 << 32):
            xs.append(_ri(rng, 1, (bx - 1 >> 32) + 1) << 32 if (bx - 1) >> 32 else 0)
            ys.append(_ri(rng, 0, min(by, R - 1)))
            kinds.append(32)
        a = _ri(rng, 0, 33)
        ux, uy = (bx - 1) >> a, (by - 1) >> (32 - a)
        if ux and uy:
            xs.append((_ri(rng, 0, ux) | 1) << a)
            ys.append((_ri(rng, 0, uy) | 1) << (32 - a))
            kinds.append(32)
    for a in range(0, 65):
        ux, uy = (bx - 1) >> a, (by - 1) >> (64 - a)
        for _ in range(4):
            if ux and uy:
                xs.append(_ri(rng, 1, ux + 1) << a)
                ys.append(_ri(rng, 1, uy + 1) << (64 - a))
                kinds.append(64)
    for v in (1, q - 1, by - 1):
        xs += [0, min(v, bx - 1)]
        ys += [min(v, by - 1), 0]
        kinds += [64, 64]
    x, y = _arr(xs), _arr(ys)
    prod = x * y
    k = np.array(kinds)
    assert max(xs) < bx and max(ys) < by
    assert not (prod & _M32)[k == 32].any() and not prod[k == 64].any()
    assert (k == 32).any() and (k == 64).any(), "the zero-round family misses a kind"
    return x, y


def _top(rng, bound, n):
    """n words in the top 1/256 of [0, bound)"""
    span = max(1, bound >> 8)
    return _arr(bound - 1 - int(v) for v in rng.integers(0, span, size=n, dtype=np.uint64))


def _hunt(rng, q, bx):
    """low words 2^32 - i against 2^32 - j (x0 w0 next to 2^64: the first carry at any q0), high words from the top and random"""
    if q <= (1 << 32) or bx <= (1 << 32):
        return _arr([bx - 1]), _arr([q - 1])
    xs, ws = [], []
    for i, j in itertools.product(range(1, 17), range(1, 17)):
        for top in (True, False):
            x1 = ((bx - 1) >> 32) - 1 if top else _ri(rng, 0, (bx - 1) >> 32)
            w1 = ((q - 1) >> 32) - 1 if top else _ri(rng, 0, (q - 1) >> 32)
            xs.append(max(x1, 0) << 32 | ((1 << 32) - i))
            ws.append(max(w1, 0) << 32 | ((1 << 32) - j))
    return _arr(xs), _arr(ws)


def _product_families(rng, q, bx, keys=False):
    """families of (x, w) for a Montgomery product with x < bx, w < q"""
    fam = {"lattice": _lattice((bx, q), q), "zero": _zero_pairs(rng, q, bx, q),
           "top": (np.concatenate([_top(rng, bx, 2048), _top(rng, bx, 2048), _uniform(rng, bx, 2048)]),
                   np.concatenate([_top(rng, q, 2048), _uniform(rng, q, 2048), _top(rng, q, 2048)])),
           "hunt": _hunt(rng, q, bx)}
    if keys:  # y at or above q while x y < q 2^64 (the RGSW kernel's key words after the lazy helpers)
        y = np.concatenate([_arr([q, q + 1, 2 * q - 1, 2 * q, 4 * q - 1, M64, M64 - 1, 1 << 63, (1 << 63) - 1]),
                            _arr(q + int(v) for v in rng.integers(0, R - q, size=4096, dtype=np.uint64))])
        lim = [min(bx, (q * R - 1) // int(v) + 1) for v in y.tolist()]  # x y < q 2^64
        half = len(lim) // 2
        x = _arr([l - 1 if i < half else _ri(rng, 0, l) for i, l in enumerate(lim)])
        assert all(int(a) * int(b) < q * R and int(b) >= q for a, b in zip(x.tolist(), y.tolist()))
        fam["keys"] = (x, y)
    fam["random"] = (_uniform(rng, bx, N_RANDOM), _uniform(rng, q, N_RANDOM))
    return fam


def _inv_pair(d, q):
    """(a, b) in [0, 2q)^2 with a + 2q - b = d, for 0 < d < 4q"""
    twoq = U(2 * q)
    a = np.where(d > twoq, d - twoq, U(0))
    return a, a + twoq - d


_SEEDS = {name: 7100 + i for i, name in enumerate(["mont", "w32", "keys", "hi128", "word", "word2", "halve", "fwd", "nc", "inv", "u52",
                                                   "modmul", "modmul_wide", "f64x"])}


def set_kind(op):
    """ops that share a domain share their operand sets"""
    return {"MRED_LAZY": "mont", "MRED": "mont", "MRED_LAZY_W32": "keys", "MRED_LAZY_ASM": "w32", "MRED128_LAZY": "hi128",
            "BRED_ADD_LAZY": "word", "BRED_ADD": "word", "MFORM_LAZY": "word", "MFORM": "word", "IMFORM_LAZY": "word", "IMFORM": "word",
            "BRED_LAZY": "word2", "BRED": "word2", "HALVE": "halve", "BFLY_FWD": "fwd", "BFLY_FWD_ASM": "fwd", "BFLY_FWD_NC": "nc",
            "BFLY_FWD_NC_ASM": "nc", "BFLY_INV": "inv", "BFLY_INV_ASM": "inv", "BFLY_INV_SCALED": "inv", "BFLY_INV_SCALED_ASM": "inv",
            "MODMUL_F64": "modmul", "REDUCE_F64": "f64x", "CANON_F64D": "f64x", "CANON_F64": "f64x", "U52_TO_F64": "u52",
            "F64_TO_U52": "u52f"}[op]


def domain(kind, q):
    """the exclusive bounds of the operands (integer kinds)"""
    B = lazy_bound(q)
    return {"mont": (R, q), "w32": (B, q), "keys": (B, R), "hi128": (q, R), "word": (R,), "word2": (R, R), "halve": (q,),
            "fwd": (4 * q, 4 * q, q), "nc": (32 * q + 1, 34 * q, q), "inv": (2 * q, 2 * q, q)}[kind]


@functools.lru_cache(None)
def families(kind, q):
    """{family: tuple of operand arrays} of one domain at one modulus; see the module docstring"""
    if kind in ("modmul", "modmul_wide", "f64x", "u52", "u52f"):
        return _f64_families(kind, q)
    rng = rng_for(_SEEDS[kind] * 100 + q % 97)
    dom = domain(kind, q)
    if kind in ("mont", "w32", "keys"):
        fam = _product_families(rng, q, lazy_bound(q) if kind != "mont" else R, keys=(kind == "keys"))
    elif kind in ("hi128", "word2"):
        fam = {"lattice": _lattice(dom, q), "zero": _zero_pairs(rng, q, dom[0], dom[1]),
               "top": (_top(rng, dom[0], 4096), _top(rng, dom[1], 4096)),
               "random": (_uniform(rng, dom[0], N_RANDOM), _uniform(rng, dom[1], N_RANDOM))}
    elif kind in ("word", "halve"):
        b = dom[0]
        fam = {"lattice": (_arr(edge_values(q, b) + [v for k in range(1, 40) for v in (k * q - 1, k * q, k * q + 1) if v < b]),),
               "zero": (_arr(v for v in (0, 1 << 32, (b - 1) >> 32 << 32, 3 << 32) if v < b),),
               "top": (_top(rng, b, 4096),), "random": (_uniform(rng, b, N_RANDOM),)}
    else:  # the butterflies: the product families feed the multiplied operand
        bx = {"fwd": 4 * q, "nc": 34 * q, "inv": 4 * q}[kind]
        prod = _product_families(rng, q, bx)
        fam = {}
        for name, (x, w) in prod.items():
            if name == "lattice":
                continue
            if kind == "inv":
                keep = x != U(0)  # a + 2q - b is never zero
                x, w = x[keep], w[keep]
                a, b = _inv_pair(x, q)
                fam[name] = (a, b, w)
            else:
                other = _uniform(rng, dom[0], len(x))
                other[: len(x) // 2] = _top(rng, dom[0], len(x) // 2)
                fam[name] = (other, x, w)
        fam = {"lattice": _lattice(dom, q), **fam}
    total = 0
    for name, cols in fam.items():
        assert len(cols) == len(dom) and len(cols[0]) > 0, f"family {name} of {kind} mod {q:#x} is empty"
        for col, b in zip(cols, dom):
            assert col.dtype == U and len(col) == len(cols[0])
            assert b >= R or (col < U(b)).all(), f"family {name} of {kind} mod {q:#x} leaves its domain"
        total += len(cols[0])
    assert total <= MAX_SET, (kind, q, total)
    return fam


A_MAGNITUDE = 36  # |a| <= 36q: a lazy input word below 2q plus the 17 stages' growth of 2q each (kernels.hip "34q + input")


def _f64_families(kind, q):
    rng = rng_for(_SEEDS.get(kind, 7190) * 100 + q % 97)
    lim = 1 << 53
    if kind in ("u52", "u52f"):
        b = 1 << 52
        vals = edge_values(q, b) + [int(v) for v in rng.integers(0, b, size=N_RANDOM, dtype=np.uint64)]
        fam = {"lattice": (_arr(edge_values(q, b)),), "random": (_arr(vals[len(edge_values(q, b)):]),)}
        return fam if kind == "u52" else {k: (f64_bits(v[0].tolist()),) for k, v in fam.items()}
    if kind == "f64x":  # x = +-(k q + delta), |x| < 2^53
        kmax = (lim - 1) // q
        ks = sorted({0, 1, 2, 3, kmax - 1, kmax, kmax // 2, (1 << 32) // q + 1} | {int(v) for v in rng.integers(0, kmax + 1, size=48)})
        deltas = [0, 1, -1, (q - 1) // 2, (q + 1) // 2, -((q - 1) // 2), -((q + 1) // 2), q - 1, -(q - 1)]
        lat = [s * (k * q + d) for k in ks for d in deltas for s in (1, -1) if abs(k * q + d) < lim]
        rnd = [int(v) - lim + 1 for v in rng.integers(0, 2 * lim - 1, size=N_RANDOM, dtype=np.uint64)]
        return {"lattice": (f64_bits(lat),), "half": (f64_bits(lat[:]),), "random": (f64_bits(rnd),)}
    amax = min(A_MAGNITUDE * q, lim - 1) if kind == "modmul" else lim - 1  # |a| <= amax
    ev = [v for v in edge_values(q, amax + 1)]
    wv = edge_values(q, q)
    lat = [(s * a, w) for a in ev for w in wv for s in (1, -1)]
    # half and whole quotients: a = ((q +- 1) / 2 + t) w^-1 + j q puts a w / q within 3 / q of a half-integer (t small), and
    # a = t w^-1 + j q of an integer
    half = []
    jmax = (amax - q) // q
    for w in [int(v) for v in rng.integers(1, q, size=1500)] + [1, 2, q - 1, q - 2, (q - 1) // 2, (q + 1) // 2]:
        winv = pow(w, -1, q)
        for base in ((q + 1) // 2, (q - 1) // 2, 0):
            for t in range(-2, 3):
                a0 = (base + t) * winv % q
                for j in (0, _ri(rng, 0, jmax + 1), jmax):
                    a = a0 + j * q
                    assert a <= amax
                    half += [(a, w), (-a, w)]
    half = half[: 1 << 15]
    rnd = [(int(a) - amax, int(w)) for a, w in zip(rng.integers(0, 2 * amax + 1, size=N_RANDOM, dtype=np.uint64).tolist(),
                                                  rng.integers(0, q, size=N_RANDOM, dtype=np.uint64).tolist())]
    fam = {}
    for name, pairs in (("lattice", lat), ("half", half), ("random", rnd)):
        assert pairs and all(abs(a) <= amax and 0 <= w < q for a, w in pairs), name
        fam[name] = (f64_bits(a for a, _ in pairs), f64_bits(w for _, w in pairs))
    return fam


def flat(kind, q):
    """(operand arrays of the whole set, [(family, first index, length)])"""
    fam = families(kind, q)
    spans, pos = [], 0
    for name, cols in fam.items():
        spans.append((name, pos, len(cols[0])))
        pos += len(cols[0])
    ncol = len(next(iter(fam.values())))
    return tuple(np.ascontiguousarray(np.concatenate([fam[n][k] for n in fam])) for k in range(ncol)), spans


def op_sets(op):
    """the set kinds an op is run on: modmul_f64 also takes the wide set (|a| < 2^53: exactness only, no magnitude claim)"""
    return ("modmul", "modmul_wide") if op == "MODMUL_F64" else (set_kind(op),)


@functools.lru_cache(None)
def reference(op, kind, q):
    """(args, spans, out0, out1) of one op on one of its sets, computed once per process"""
    args, spans = flat(kind, q)
    out0, out1 = expected(op, q, args)
    for a in args + (out0,) + ((out1,) if out1 is not None else ()):
        a.setflags(write=False)
    return args, spans, out0, out1


def product_operands(op, kind, q):
    """the (x, w) an op of the word-serial schedules hands its product(s), for the carry counts"""
    args, _ = flat(kind, q)
    if op in ("MRED_LAZY_W32", "MRED_LAZY_ASM"):
        return [(args[0], args[1])]
    a, b, w = args
    if op in ("BFLY_FWD", "BFLY_FWD_ASM") or op in NC_OPS:
        return [(b, w)]
    twoq, x = U(2 * q), a + b
    if op == "BFLY_INV_ASM":
        return [(a + twoq - b, w)]
    if op == "BFLY_INV_SCALED_ASM":
        return [(np.where(x >= twoq, x - twoq, x), np.full_like(a, consts(q).ninv)), (a + twoq - b, w)]
    return []


def first_difference(op, name, q, spans, args, got, want):
    """the failure message of a comparison: op, modulus, family and the first differing tuple in hex"""
    i = int(np.flatnonzero(got != want)[0])
    fam = next(f for f, s, n in spans if s <= i < s + n)
    return (f"{op} mod {name} = {q:#x}, family {fam}, tuple {i}: (" + ", ".join(f"{int(a[i]):#x}" for a in args)
            + f") -> {int(got[i]):#x}, expected {int(want[i]):#x}; {int((got != want).sum())} of {len(want)} differ")


# ---------------------------------------------------------------------------------------------------------------
# auto_dest
# ---------------------------------------------------------------------------------------------------------------
def auto_dest_cases():
    """(logN, g): g in {5, 5^k, 2N - 1} for logN 12 .. 17"""
    out = []
    for logn in range(12, 18):
        n2 = 2 << logn
        out += [(logn, 5), (logn, pow(5, 3 + 7 * logn, n2)), (logn, n2 - 1)]
    return out


def auto_dest_reference(logn, g):
    """(e, ginv, logN) for every e and the destinations: the inverse of the oracle's AutomorphismNTTIndex -- the automorphism is
    the gather out[j] = in[index[j]], so source coefficient e lands at the j with index[j] = e"""
    n = 1 << logn
    idx = O.AutomorphismNTTIndex(n, 2 * n, g).astype(np.int64)
    dest = np.empty(n, dtype=U)
    dest[idx] = np.arange(n, dtype=U)
    assert sorted(idx.tolist()) == list(range(n))
    e = np.arange(n, dtype=U)
    return (e, np.full(n, pow(g, -1, 2 * n), dtype=U), np.full(n, logn, dtype=U)), dest
