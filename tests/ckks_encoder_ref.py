"""Restatement of the double-precision path of the reference's ckks.Encoder (schemes/ckks/encoder.go, ckks_vector_ops.go,
utils.go, scaling.go:46, core/rlwe/utils.go:187) in numpy / Python, for the tests of include/hering_ckks_encoder.h.

Real and imaginary parts are separate float64 arrays and every written operation of the reference is ONE numpy operation: numpy's
complex multiply and divide are never used (their rounding is the C compiler's choice).  Conversions from float to integer at or
above 2^63 and from big integers to float go through Python int / float (exact, round-to-nearest-even).  Every function takes the
table of roots as an argument (re, im: float64 [M + 1])."""
from __future__ import annotations

import math

import numpy as np

GALOIS_GEN = 5


def roots_ref(M: int, cos=math.cos):
    """GetRootsComplex128(M) (utils.go:53-77) with the given cosine: (re, im) float64 [M + 1]."""
    re, im = np.zeros(M + 1), np.zeros(M + 1)
    quarm = M >> 2
    angle = 2 * 3.141592653589793 / float(M)
    for i in range(quarm):
        re[i] = cos(angle * float(i))
    for i in range(quarm):
        re[quarm - i] += 0.0
        im[quarm - i] += re[i]
    for i in range(1, quarm + 1):
        re[i + quarm], im[i + quarm] = -re[quarm - i], im[quarm - i]
        re[i + 2 * quarm], im[i + 2 * quarm] = -re[i], -im[i]
        re[i + 3 * quarm], im[i + 3 * quarm] = re[quarm - i], -im[quarm - i]
    re[M], im[M] = re[0], im[0]
    return re, im


def rot_group(M: int) -> np.ndarray:
    """rotGroup[j] = 5^j mod M (encoder.go:83-89)"""
    out = np.zeros(M >> 2, dtype=np.int64)
    five = 1
    for i in range(M >> 2):
        out[i] = five
        five = (five * GALOIS_GEN) & (M - 1)
    return out


def bit_reverse(n: int) -> np.ndarray:
    logn = n.bit_length() - 1
    idx = np.arange(n)
    out = np.zeros(n, dtype=np.int64)
    for b in range(logn):
        out |= ((idx >> b) & 1) << (logn - 1 - b)
    return out


def _cmul(ar, ai, br, bi):
    """(a + bi)(c + di) = (ac - bd) + (ad + bc)i, four products, one difference, one sum"""
    return ar * br - ai * bi, ar * bi + ai * br


def _stage(loglen, n, M, rot):
    """index arrays of one stage: k, k + lenh and the twiddle exponents (forward, inverse)"""
    logM = M.bit_length() - 1
    ln, lenh, lenq = 1 << loglen, 1 << (loglen - 1), 4 << loglen
    log_gap, mask = logM - 2 - loglen, lenq - 1
    t = np.arange(n >> 1)
    j = t & (lenh - 1)
    k = (t >> (loglen - 1)) * ln + j
    r = rot[j] & mask
    return k, k + lenh, r << log_gap, (lenq - r) << log_gap


def special_fft(re, im, M, rre, rim):
    """SpecialFFTDouble (ckks_vector_ops.go:50-76) of n = len(re) values; returns new arrays"""
    n = len(re)
    rot = rot_group(M)
    br = bit_reverse(n)
    re, im = np.array(re, dtype=np.float64)[br], np.array(im, dtype=np.float64)[br]
    for loglen in range(1, n.bit_length()):
        k, kh, wf, _ = _stage(loglen, n, M, rot)
        pr, pi = _cmul(re[kh], im[kh], rre[wf], rim[wf])
        ur, ui = re[k].copy(), im[k].copy()
        re[k], im[k] = ur + pr, ui + pi
        re[kh], im[kh] = ur - pr, ui - pi
    return re, im


def special_ifft(re, im, M, rre, rim):
    """SpecialIFFTDouble (:18-47)"""
    n = len(re)
    rot = rot_group(M)
    re, im = np.array(re, dtype=np.float64), np.array(im, dtype=np.float64)
    for loglen in range(n.bit_length() - 1, 0, -1):
        k, kh, _, wi = _stage(loglen, n, M, rot)
        ur, ui, vr, vi = re[k].copy(), im[k].copy(), re[kh].copy(), im[kh].copy()
        re[k], im[k] = ur + vr, ui + vi
        re[kh], im[kh] = _cmul(ur - vr, ui - vi, rre[wi], rim[wi])
    # values[i] /= complex(float64(N), 0): two real divisions for finite input (the sign of a zero result aside)
    re, im = re / float(n), im / float(n)
    br = bit_reverse(n)
    return re[br], im[br]


def _unrolled_pairs(loglen, n):
    """the butterflies (j, k) of one stage in the order of the unrolled schedules (SpecialFFTDoubleUL8 :160-339,
    SpecialiFFTDoubleUnrolled8 :342-477): chunks of 8 for lenh > 8, blocks of 16 values below"""
    ln, lenh = 1 << loglen, 1 << (loglen - 1)
    if lenh > 8:
        for i in range(0, n, ln):
            for j in range(0, lenh, 8):
                for u in range(8):
                    yield j + u, i + j + u
    else:
        for i in range(0, n, 16):
            for blk in range(0, 16, ln):
                for j in range(lenh):
                    yield j, i + blk + j


def special_fft_unrolled(re, im, M, rre, rim):
    """SpecialFFTDoubleUL8, butterfly by butterfly in its own order (n >= 16)"""
    n = len(re)
    assert n >= 16
    rot = rot_group(M)
    logM = M.bit_length() - 1
    br = bit_reverse(n)
    re, im = np.array(re, dtype=np.float64)[br], np.array(im, dtype=np.float64)[br]
    for loglen in range(1, n.bit_length()):
        lenh, lenq = 1 << (loglen - 1), 4 << loglen
        log_gap, mask = logM - 2 - loglen, lenq - 1
        for j, k in _unrolled_pairs(loglen, n):
            w = (int(rot[j]) & mask) << log_gap
            vr, vi = _cmul(re[k + lenh], im[k + lenh], rre[w], rim[w])
            ur, ui = re[k], im[k]
            re[k], im[k] = ur + vr, ui + vi
            re[k + lenh], im[k + lenh] = ur - vr, ui - vi
    return re, im


def special_ifft_unrolled(re, im, M, rre, rim):
    """SpecialiFFTDoubleUnrolled8 (n >= 16)"""
    n = len(re)
    assert n >= 16
    rot = rot_group(M)
    logM = M.bit_length() - 1
    re, im = np.array(re, dtype=np.float64), np.array(im, dtype=np.float64)
    for loglen in range(n.bit_length() - 1, 0, -1):
        lenh, lenq = 1 << (loglen - 1), 4 << loglen
        log_gap, mask = logM - 2 - loglen, lenq - 1
        for j, k in _unrolled_pairs(loglen, n):
            w = (lenq - (int(rot[j]) & mask)) << log_gap
            ur, ui, vr, vi = re[k], im[k], re[k + lenh], im[k + lenh]
            re[k], im[k] = ur + vr, ui + vi
            re[k + lenh], im[k + lenh] = _cmul(ur - vr, ui - vi, rre[w], rim[w])
    re, im = re / float(n), im / float(n)
    br = bit_reverse(n)
    return re[br], im[br]


# ---- the quantiser ----------------------------------------------------------------------------------------------------------
def bred_add(c: int, q: int) -> int:
    """ring.BRedAdd: c mod q for a 64-bit c"""
    return c % q


def quantise_word(value: float, scale: float, q: int) -> int:
    """SingleFloat64ToFixedPointCRT (utils.go:171-234) for one modulus"""
    value, scale = float(value), float(scale)
    if value == 0:
        return 0
    neg = value < 0
    if neg:
        scale *= -1
    value *= scale
    if value >= 1.8446744073709552e+19:
        # big.NewFloat(value) + 0.5 at 53 bits rounds back to value (its ulp is 2^12 or more); Int truncates: the integer is value
        x = int(value)
        return q - x % q if neg else x % q
    c = int(value + 0.5)  # uint64(value + 0.5): a float64 add, then truncation
    if neg:
        return q - bred_add(c, q) if c > q else q - c
    return bred_add(c, q) if c > 0x1FFFFFFFFFFFFFFF else c


def quantise_poly(values, scale, moduli, N) -> np.ndarray:
    """words [limbs][N] of the coefficients `values` (the rest zero)"""
    out = np.zeros((len(moduli), N), dtype=np.uint64)
    for i, v in enumerate(values):
        if v != 0:
            for l, q in enumerate(moduli):
                out[l, i] = quantise_word(v, scale, q)
    return out


def embed_coeffs(values, log_slots, N, conjugate_invariant, M, rre, rim):
    """embedDouble (encoder.go:216-337) up to the quantiser's input: the N coefficient values in position (stride gap), as the
    device writes them for a polynomial in Y = X^gap.  values: complex or real, zero-padded to slots."""
    slots = 1 << log_slots
    v = np.zeros(slots, dtype=np.complex128)
    v[: len(values)] = values
    re, im = v.real.copy(), (np.zeros(slots) if conjugate_invariant else v.imag.copy())
    re, im = special_ifft(re, im, M, rre, rim)  # (the unrolled schedule gives the same words: test_ckks_encoder_host)
    max_slots = M >> 2
    gap = max_slots // slots
    out = np.zeros(N)
    out[0: slots * gap: gap] = re
    if not conjugate_invariant:
        out[N // 2: N // 2 + slots * gap: gap] = im
    return out


# ---- reconstruction ----------------------------------------------------------------------------------------------------------
def crt(residues, moduli) -> int:
    Q = 1
    for q in moduli:
        Q *= q
    x = 0
    for r, q in zip(residues, moduli):
        Qi = Q // q
        x += int(r) * Qi * pow(Qi, -1, q)
    return x % Q


def coeff_to_float(residues, moduli, scale: float) -> float:
    """polyToComplexCRT / polyToFloatCRT with scaleDown (encoder.go:924-1116, scaling.go:46): the exact integer mod Q, centred with
    x >= Q >> 1 -> x - Q, rounded to nearest-even (Python's int -> float), divided by the scale.  One limb: the same value as
    polyToFloatNoCRT's -float64(Q - c) / float64(c)."""
    Q = 1
    for q in moduli:
        Q *= q
    x = crt(residues, moduli)
    if x >= Q >> 1:
        x -= Q
    try:
        f = float(x)
    except OverflowError:
        f = math.inf if x > 0 else -math.inf
    return f / float(scale)


def go_round(x: float) -> float:
    """math.Round: to the nearest integer, halves away from zero (the fraction of a float64 is exact)"""
    a = abs(x)
    if a >= 4503599627370496.0 or a != a:
        return x
    f = math.floor(a)
    if a - f >= 0.5:
        f += 1.0
    return math.copysign(f, x)


def decode_slots(coeffs, moduli, scale, log_slots, N, conjugate_invariant, M, rre, rim, logprec=0.0, fft=True):
    """decodePublic (encoder.go:497-760), batched: coeffs [limbs][N] coefficient domain -> (re, im) of the slots"""
    slots = 1 << log_slots
    gap = (M >> 2) // slots
    re = np.array([coeff_to_float(coeffs[:, i * gap], moduli, scale) for i in range(slots)])
    if not conjugate_invariant:
        im = np.array([coeff_to_float(coeffs[:, N // 2 + i * gap], moduli, scale) for i in range(slots)])
    else:
        # for i := 1; i < slots; i++ { values[i] -= complex(0, real(values[slots-i])) }
        im = np.zeros(slots)
        for i in range(1, slots):
            im[i] -= re[slots - i]
    if fft:
        re, im = special_fft(re, im, M, rre, rim)
    if logprec != 0:
        s = math.pow(2.0, logprec)  # math.Exp2 (exact for the integral logprec the tests use)
        re, im = np.array([go_round(x * s) / s for x in re]), np.array([go_round(x * s) / s for x in im])
    return re, im


# ---- the edge lists of the tests (host and device) -----------------------------------------------------------------------------
def quantiser_cases(q):
    """(value, scale) pairs of the edge list; c and v of the comments are |value scale| as the rule names them"""
    cases = [(0.0, 1.0), (-0.0, 1.0), (-0.25, 1.0)]  # (a negative value with c = 0: the word q)
    # a product that is zero although the value is not (scale 0, underflow): c = uint64(0.5) = 0, the word q for a negative value
    cases += [(1.0, 0.0), (-1.0, 0.0), (1e-300, 1e-30), (-1e-300, 1e-30)]
    for v in (0.49999999999999994, 0.5, 1.5, 2.5):
        cases += [(v, 1.0), (-v, 1.0)]
    for c in (q - 1, q, q + 1, 3 * q):
        if c.bit_length() <= 53:  # c itself is a float64: exactly this c, directly and through a power-of-two scale
            cases += [(float(c), 1.0), (-float(c), 1.0), (float(c) / 4.0, 4.0), (-float(c) / 4.0, 4.0)]
        else:  # (the 61-bit prime) c is no float64: the float64 next below it and the one next above, on both sides of `c > q`
            sh = c.bit_length() - 53
            lo = float((c >> sh) << sh)
            for val in (lo, math.nextafter(lo, math.inf)):
                cases += [(val, 1.0), (-val, 1.0)]
    if q < 1 << 60:
        cases += [(float(q + 12345), 1.0), (float(1 << 60) + 4096.0, 1.0), (float(3 * q + 1), 1024.0)]  # positive c in (q, 2^61): unreduced
    cases += [(float(0x2000000000000000), 1.0), (float(0x2000000000000000) + 1024.0, 1.0), (-(float(0x2000000000000000) + 1024.0), 1.0)]
    below = math.nextafter(2.0 ** 64, 0.0)
    for v in (below, 2.0 ** 64, 2.0 ** 200, math.nextafter(2.0 ** 64, math.inf)):
        cases += [(v, 1.0), (-v, 1.0), (v / 2.0 ** 40, 2.0 ** 40)]
    # a v >= 2^64 divisible by q, of both signs: q 2^64, where q fits the 53-bit significand (no such float64 exists for a prime of
    # more than 53 bits: q would have to divide the significand)
    if q.bit_length() <= 53:
        cases += [(-float(q) * 2.0 ** 64, 1.0), (float(q) * 2.0 ** 64, 1.0)]
    return cases


def reconstruction_cases(Q):
    xs = [0, 1, -1, (Q >> 1) - 1, Q >> 1, Q - 1]
    for x in (2 ** 53 + 1, 2 ** 53 + 3, 2 ** 54 + 2, 2 ** 54 + 6, 2 ** 100 + 2 ** 47, 2 ** 100 + 2 ** 47 + 1):
        xs += [x, -x]
    return xs
