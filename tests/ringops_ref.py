"""The coefficient-wise ring operations of the reference, restated in Python integers (host only).

One function per formula of ring/vec_ops.go and ring/operations.go that the library exposes, every word computed mod 2^64 the
way the reference's wrapping uint64 arithmetic does, so that each result is defined for ANY 64-bit operand word -- the lazy
forms' real operands are words in [q, 4q) and accumulators that wrap.  Written from the reference's sources (the line of each
formula is in its comment), not from csrc/kernels.hip or oracle/lattigo_oracle.c: tests/test_ringops_host.py holds the oracle
against this file, and tests/test_gpu_ringops_edges.py holds the device against the oracle.

The word-level reductions (MRed, MRedLazy, BRed, BRedLazy, BRedAdd, BRedAddLazy, MForm, MFormLazy, IMForm, CRed) are here as
well, as the bits.Mul64 / bits.Add64 sequences of ring/modular_reduction.go: tests/arith_ref.py holds their claims (residue
class, range) and takes their WORDS from the oracle, so it has no integer form of them to build on.  tests/test_ringops_host.py
checks these against arith_ref.check_truth.

A polynomial is a list of limbs, a limb a list of Python ints; the polynomial-level functions take numpy arrays [limbs][N] and
`arr` turns a result back into one."""
from __future__ import annotations

import numpy as np

R = 1 << 64
M64 = R - 1


# ---------------------------------------------------------------------------------------------------------------
# ring/modular_reduction.go, word for word
# ---------------------------------------------------------------------------------------------------------------
class K:
    """the constants of one SubRing: Modulus, MRedConstant (modular_reduction.go:68), BRedConstant (:99)"""

    __slots__ = ("q", "qinv", "b0", "b1")
    _cache: dict = {}

    def __new__(cls, q):
        k = cls._cache.get(q)
        if k is None:
            k = object.__new__(cls)
            k.q = q
            k.qinv = pow(q, -1, R)  # :68-75, q^(2^63 - 1) mod 2^64: the inverse of the odd q
            b = (1 << 128) // q  # :99-107
            k.b0, k.b1 = b >> 64, b & M64
            cls._cache[q] = k
        return k


def CRed(a, q):  # :200
    return a - q if a >= q else a


def MRedLazy(x, y, k):  # :90
    m = x * y
    ahi, alo = m >> 64, m & M64
    H = (((alo * k.qinv) & M64) * k.q) >> 64
    return (ahi - H + k.q) & M64


def MRed(x, y, k):  # :78
    return CRed(MRedLazy(x, y, k), k.q)


def BRedAddLazy(x, k):  # :121
    return (x - ((x * k.b0) >> 64) * k.q) & M64


def BRedAdd(x, k):  # :110
    return CRed(BRedAddLazy(x, k), k.q)


def BRedLazy(x, y, k):  # :166
    m = x * y
    mhi, mlo = m >> 64, m & M64
    r = mhi * k.b0  # (wraps below, as the reference's uint64 r does)
    h = mlo * k.b0
    hhi, hlo = h >> 64, h & M64
    r += hhi
    lhi = (mlo * k.b1) >> 64
    s0 = hlo + lhi
    r += s0 >> 64
    s0 &= M64
    h = mhi * k.b1
    hhi, hlo = h >> 64, h & M64
    r += hhi
    r += (hlo + s0) >> 64
    return (mlo - r * k.q) & M64


def BRed(x, y, k):  # :127
    return CRed(BRedLazy(x, y, k), k.q)


def MFormLazy(a, k):  # :40
    return (-(a * k.b0 + ((a * k.b1) >> 64)) * k.q) & M64


def MForm(a, k):  # :11
    return CRed(MFormLazy(a, k), k.q)


def IMFormLazy(a, k):  # :61
    return (k.q - ((((a * k.qinv) & M64) * k.q) >> 64)) & M64


def IMForm(a, k):  # :49
    return CRed(IMFormLazy(a, k), k.q)


# ---------------------------------------------------------------------------------------------------------------
# ring/vec_ops.go: z = f(x, y, z) per word.  (name -> (function, reads the destination))
# ---------------------------------------------------------------------------------------------------------------
BINARY = {
    "Add": lambda x, y, z, k: CRed((x + y) & M64, k.q),  # vec_ops.go:20
    "AddLazy": lambda x, y, z, k: (x + y) & M64,  # :44
    "Sub": lambda x, y, z, k: CRed((x + k.q - y) & M64, k.q),  # :68
    "SubLazy": lambda x, y, z, k: (x + k.q - y) & M64,  # :92
    "MulCoeffsBarrett": lambda x, y, z, k: BRed(x, y, k),  # :230
    "MulCoeffsBarrettLazy": lambda x, y, z, k: BRedLazy(x, y, k),  # :254
    "MulCoeffsBarrettThenAdd": lambda x, y, z, k: CRed((z + BRed(x, y, k)) & M64, k.q),  # :278
    "MulCoeffsBarrettThenAddLazy": lambda x, y, z, k: (z + BRed(x, y, k)) & M64,  # :302
    "MulCoeffsMontgomery": lambda x, y, z, k: MRed(x, y, k),  # :325
    "MulCoeffsMontgomeryLazy": lambda x, y, z, k: MRedLazy(x, y, k),  # :349
    "MulCoeffsMontgomeryLazyThenNeg": lambda x, y, z, k: (2 * k.q - MRedLazy(x, y, k)) & M64,  # :518
    "MulCoeffsMontgomeryThenAdd": lambda x, y, z, k: CRed((z + MRed(x, y, k)) & M64, k.q),  # :372
    "MulCoeffsMontgomeryThenAddLazy": lambda x, y, z, k: (z + MRed(x, y, k)) & M64,  # :396
    "MulCoeffsMontgomeryLazyThenAddLazy": lambda x, y, z, k: (z + MRedLazy(x, y, k)) & M64,  # :420
    "MulCoeffsMontgomeryThenSub": lambda x, y, z, k: CRed((z + (k.q - MRed(x, y, k))) & M64, k.q),  # :444
    "MulCoeffsMontgomeryThenSubLazy": lambda x, y, z, k: (z + (k.q - MRed(x, y, k))) & M64,  # :468
    "MulCoeffsMontgomeryLazyThenSubLazy": lambda x, y, z, k: (z + ((2 * k.q - MRedLazy(x, y, k)) & M64)) & M64,  # :493
}
READS_Z = {n for n in BINARY if "Then" in n and not n.endswith("ThenNeg")}
UNARY = {
    "Neg": lambda x, k: (k.q - x) & M64,  # :114
    "Reduce": lambda x, k: BRedAdd(x, k),  # :136
    "ReduceLazy": lambda x, k: BRedAddLazy(x, k),  # :158
    "MForm": lambda x, k: MForm(x, k),  # :789
    "MFormLazy": lambda x, k: MFormLazy(x, k),  # :811
    "IMForm": lambda x, k: IMForm(x, k),  # :833
}
# the SubRing scalar forms Ring.*Scalar* call: z = f(x, prepared scalar, z)
_add_scalar = lambda x, s, z, k: CRed((x + s) & M64, k.q)  # :586
_sub_scalar = lambda x, s, z, k: CRed((x + k.q - s) & M64, k.q)  # :653
_mul_scalar = lambda x, s, z, k: MRed(x, s, k)  # :675
_mul_scalar_then_add = lambda x, s, z, k: CRed((z + MRed(x, s, k)) & M64, k.q)  # :719
# ring/operations.go: (how Ring.X prepares its uint64 scalar for limb i, the SubRing form it calls)
SCALAR = {
    "AddScalar": (lambda s, k: s, _add_scalar),  # operations.go:151 (the scalar goes in unreduced)
    "SubScalar": (lambda s, k: s, _sub_scalar),  # :186
    "MulScalar": (lambda s, k: MForm(s, k), _mul_scalar),  # :201
    "MulScalarThenAdd": (lambda s, k: MForm(s, k), _mul_scalar_then_add),  # :208
    "MulScalarThenSub": (lambda s, k: MForm((k.q - BRedAdd(s, k)) & M64, k), _mul_scalar_then_add),  # :223
}
SCALAR_READS_Z = {"MulScalarThenAdd", "MulScalarThenSub"}
# big.Int.Mod is Euclidean, and so is Python's % for a positive modulus
BIGINT = {
    "AddScalarBigint": (lambda s, k: s % k.q, _add_scalar),  # :158
    "SubScalarBigint": (lambda s, k: s % k.q, _sub_scalar),  # :193
    "MulScalarBigint": (lambda s, k: MForm(s % k.q, k), _mul_scalar),  # :231
    "MulScalarBigintThenAdd": (lambda s, k: MForm(s % k.q, k), _mul_scalar_then_add),  # :240
}
# scalar0[i] on the coefficients [0, N/2), scalar1[i] on [N/2, N)
DOUBLE = {
    "AddDoubleRNSScalar": (lambda s, k: s, _add_scalar),  # :167
    "SubDoubleRNSScalar": (lambda s, k: s, _sub_scalar),  # :177
    "MulDoubleRNSScalar": (lambda s, k: MForm(s, k), _mul_scalar),  # :250
    "MulDoubleRNSScalarThenAdd": (lambda s, k: MForm(s, k), _mul_scalar_then_add),  # :260
}


def _rows(a):
    return np.asarray(a, dtype=np.uint64).tolist()


def binop(name, mods, x, y, z=None):
    """Ring.<name>(p1, p2, p3) on limbs 0..len(mods)-1 (operations.go:11-148)"""
    f = BINARY[name]
    x, y = _rows(x), _rows(y)
    z = _rows(z) if z is not None else [[0] * len(r) for r in x]
    return [[f(a, b, c, K(q)) for a, b, c in zip(x[i], y[i], z[i])] for i, q in enumerate(mods)]


def unop(name, mods, x):
    f = UNARY[name]
    x = _rows(x)
    return [[f(a, K(q)) for a in x[i]] for i, q in enumerate(mods)]


def _scalar(table, name, mods, x, scalars, z):
    prep, f = table[name]
    x = _rows(x)
    z = _rows(z) if z is not None else [[0] * len(r) for r in x]
    out = []
    for i, q in enumerate(mods):
        k = K(q)
        s = prep(scalars[i], k)
        out.append([f(a, s, c, k) for a, c in zip(x[i], z[i])])
    return out


def scalarop(name, mods, x, scalar, z=None):
    """Ring.<name>(p1, scalar uint64, p2) (operations.go:151, 186, 201, 208, 223)"""
    return _scalar(SCALAR, name, mods, x, [int(scalar)] * len(mods), z)


def bigintop(name, mods, x, scalar, z=None):
    """Ring.<name>(p1, scalar *big.Int, p2) (operations.go:158, 193, 231, 240)"""
    return _scalar(BIGINT, name, mods, x, [int(scalar)] * len(mods), z)


def MulRNSScalarMontgomery(mods, x, scalar):
    """operations.go:216: the per-limb word goes to MRed as it is"""
    x = _rows(x)
    return [[MRed(a, int(scalar[i]), K(q)) for a in x[i]] for i, q in enumerate(mods)]


def doubleop(name, mods, x, scalar0, scalar1, z=None):
    """Ring.{Add,Sub,Mul}DoubleRNSScalar[ThenAdd] (operations.go:167-184, 250-266)"""
    a = _scalar(DOUBLE, name, mods, x, [int(s) for s in scalar0], z)
    b = _scalar(DOUBLE, name, mods, x, [int(s) for s in scalar1], z)
    h = len(a[0]) >> 1
    return [ra[:h] + rb[h:] for ra, rb in zip(a, b)]


def MulByVectorMontgomery(mods, x, vector, z=None):
    """operations.go:366 (z given: MulByVectorMontgomeryThenAddLazy :373): the same vector against every limb"""
    v = [_rows(vector)] * len(mods)
    return binop("MulCoeffsMontgomery" if z is None else "MulCoeffsMontgomeryThenAddLazy", mods, x, v, z)


# ---------------------------------------------------------------------------------------------------------------
# the permutations
# ---------------------------------------------------------------------------------------------------------------
def Shift(x, k):
    """operations.go:278 -> utils.RotateSliceAllocFree (utils/slices.go:77-98): k mod N taken non-negative, out = s[k:] + s[:k]"""
    x = _rows(x)
    n = len(x[0])
    k = k % n  # (Go's % truncates and :88-90 adds N to a negative remainder: the non-negative residue, as Python's)
    return [r[k:] + r[:k] for r in x]


def MultByMonomial(mods, x, k):
    """operations.go:306-363, loop for loop; the negations are q - c, so a zero word comes out as q.  (The reference indexes out
    of range for k < -2N unless 2N divides k; the callers keep to k >= -2N or such multiples.)"""
    x = _rows(x)
    N = len(x[0])
    shift = (k + 2 * N) % (2 * N)
    if shift == 0:  # :312
        return [list(r) for r in x]
    out = []
    for i, q in enumerate(mods):
        tmp = list(x[i]) if shift < N else [(q - c) & M64 for c in x[i]]  # :325-343
        s = shift % N  # :345
        out.append([(q - tmp[N - s + j]) & M64 for j in range(s)] + tmp[: N - s])  # :347-361
    return out


def AutomorphismMap(N, gen, conjugate_invariant=False):
    """[(destination, source, negated)] of automorphism.go:113-176, index arithmetic in wrapping uint64"""
    out = []
    if conjugate_invariant:  # :122-154
        mask, logn = 2 * N - 1, (2 * N - 1).bit_length()
        for i in range(2 * N):
            raw = (i * gen) & M64
            index, tmp = raw & mask, (raw >> logn) & 1
            if index < N:
                idx = i
                if idx >= N:
                    idx, tmp = 2 * N - idx, tmp ^ 1
                out.append((index, idx, tmp))
    else:  # :156-174
        mask, logn = N - 1, (N - 1).bit_length()
        for i in range(N):
            raw = (i * gen) & M64
            out.append((raw & mask, i, (raw >> logn) & 1))
    return out


def Automorphism(mods, x, gen, conjugate_invariant=False):
    """automorphism.go:113-176 in the coefficient domain, both ring types: out[index] = in[idx] (1 - tmp) | (q - in[idx]) tmp
    (:151, :172) -- a negated zero word comes out as q"""
    x = _rows(x)
    N = len(x[0])
    out = [[None] * N for _ in mods]
    for index, idx, tmp in AutomorphismMap(N, gen, conjugate_invariant):
        for j, q in enumerate(mods):
            out[j][index] = (q - x[j][idx]) & M64 if tmp else x[j][idx]
    assert all(v is not None for r in out for v in r), "not a permutation (an even Galois element?)"
    return out


def _bitrev(x, bits):
    r = 0
    for _ in range(bits):
        r, x = (r << 1) | (x & 1), x >> 1
    return r


def AutomorphismNTTIndex(N, nth_root, gal):
    """automorphism.go:12-34"""
    log_nth_root = (nth_root - 1).bit_length() - 1
    mask = nth_root - 1
    out = []
    for i in range(N):
        t1 = 2 * _bitrev(i, log_nth_root) + 1
        t2 = ((((gal * t1) & M64) & mask) - 1) >> 1
        out.append(_bitrev(t2, log_nth_root))
    return out


def AutomorphismNTTWithIndex(x, index, z=None):
    """automorphism.go:50 (z given: ...ThenAddLazy :82, a wrapping +=)"""
    x = _rows(x)
    if z is None:
        return [[r[int(s)] for s in index] for r in x]
    z = _rows(z)
    return [[(c + r[int(s)]) & M64 for c, s in zip(zr, index)] for r, zr in zip(x, z)]


def arr(p):
    """a polynomial of this module as a numpy [limbs][N] uint64 array"""
    return np.array(p, dtype=np.uint64)
