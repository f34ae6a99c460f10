"""The restatement of the reference's double-precision ckks.Encoder (tests/ckks_encoder_ref.py) against definitions that do not
share its code: the special FFT against the O(n^2) sum at 100 digits, the quantiser and the reconstruction against big-integer
statements of their rules on the edge lists, the built-in table of roots of libhering.so (he_ckks_roots_host, no device needed)
against the structure of GetRootsComplex128, and the wiring of include/hering_ckks_encoder.h.  No GPU."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
from fractions import Fraction

import mpmath
import numpy as np
import pytest

from lattigo_amd import _lib
from oracle import oracle as O
from tests import ckks_encoder_ref as R
from tests.helpers import rng_for
from tests.rlwe_fixtures import downstream_primes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hering_ckks_encoder.h")
NEW = ["he_ckks_roots_host", "he_ckks_encoder_create", "he_ckks_encoder_destroy", "he_ckks_encoder_roots", "he_ckks_encoder_info", "he_ckks_fft",
       "he_ckks_ifft", "he_ckks_encode", "he_ckks_encode_qp", "he_ckks_decode"]
U = 2.0 ** -53  # unit roundoff


def lib_roots(M):
    out = np.zeros(2 * (M + 1))
    rc = _lib.load().he_ckks_roots_host(M, out.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0
    return out[0::2].copy(), out[1::2].copy()


def fft_bound(n):
    """Higham, Accuracy and Stability of Numerical Algorithms, Theorem 24.2: a radix-2 FFT of n = 2^t values with twiddles of
    absolute error mu has || y^ - y ||_2 <= t eta / (1 - t eta) || y ||_2, eta = mu + gamma_4 (sqrt 2 + mu), gamma_4 = 4u / (1 - 4u).
    mu: the argument angle * i carries three roundings (2 pi, the division, the product) on a value below pi / 2, so at most 5u in
    the cosine, plus one ulp of the library's: 6u per part, 6 sqrt 2 u < 9u for the complex root."""
    t = max(n.bit_length() - 1, 1)
    mu, g4 = 9 * U, 4 * U / (1 - 4 * U)
    eta = mu + g4 * (math.sqrt(2) + mu)
    return t * eta / (1 - t * eta)


def definition_fft(re, im, n):
    """z_j = sum_k w_k zeta^(5^j k), zeta = exp(2 pi i / 4n), at 100 digits"""
    mpmath.mp.dps = 100
    w = [mpmath.mpc(float(a), float(b)) for a, b in zip(re, im)]
    pw = [mpmath.expjpi(mpmath.mpf(2 * e) / (4 * n)) for e in range(4 * n)]
    out, five = [], 1
    for _ in range(n):
        out.append(mpmath.fsum(w[k] * pw[(five * k) % (4 * n)] for k in range(n)))
        five = (five * 5) % (4 * n)
    return out


@pytest.mark.parametrize("sparse", [0, 2])
@pytest.mark.parametrize("logN", [4, 5, 6, 7, 8])
def test_restated_fft_matches_the_definition(logN, sparse):
    M = 2 << logN
    n = (M >> 2) >> sparse
    rre, rim = lib_roots(M)
    rng = rng_for(4100 + logN)
    re, im = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    fr, fi = R.special_fft(re, im, M, rre, rim)
    want = definition_fft(re, im, n)
    err = math.sqrt(sum(float(abs(mpmath.mpc(a, b) - z) ** 2) for a, b, z in zip(fr, fi, want)))
    norm = math.sqrt(sum(float(abs(z) ** 2) for z in want))
    print(f"logN {logN} n {n}: relative error {err / norm:.3e}, bound {fft_bound(n):.3e}")
    assert err <= fft_bound(n) * norm
    br, bi = R.special_ifft(fr, fi, M, rre, rim)
    back = math.hypot(np.linalg.norm(br - re), np.linalg.norm(bi - im))
    print(f"logN {logN} n {n}: round trip relative error {back / math.hypot(np.linalg.norm(re), np.linalg.norm(im)):.3e}")
    assert back <= fft_bound(n) * math.hypot(np.linalg.norm(re), np.linalg.norm(im))  # IFFT . FFT = identity to the same bound


@pytest.mark.parametrize("logN,sparse", [(6, 0), (7, 0), (7, 1), (8, 2), (10, 0), (10, 1)])  # n >= 16: where the reference unrolls
def test_plain_and_unrolled_schedules_give_equal_words(logN, sparse):
    M = 2 << logN
    n = (M >> 2) >> sparse
    rre, rim = lib_roots(M)
    rng = rng_for(4200 + logN)
    re, im = rng.uniform(-8, 8, n), rng.uniform(-8, 8, n)
    for plain, unrolled in ((R.special_fft, R.special_fft_unrolled), (R.special_ifft, R.special_ifft_unrolled)):
        a, b = plain(re, im, M, rre, rim), unrolled(re, im, M, rre, rim)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("M", [32, 64, 1 << 11, 1 << 13])
def test_roots_table_has_the_reference_structure(M):
    re, im = lib_roots(M)
    bits = lambda a: np.asarray(a, dtype=np.float64).view(np.uint64)
    q = M >> 2
    assert re[0] == 1.0 and im[0] == 0.0 and re[M] == re[0] and im[M] == im[0]
    # the same copies and negations as the restatement makes of the same first quarter (bitwise)
    wre, wim = R.roots_ref(M, cos=lambda x, _t={}: re[round(x / (2 * 3.141592653589793 / float(M)))])
    assert np.array_equal(bits(re), bits(wre)) and np.array_equal(bits(im), bits(wim))
    i = np.arange(1, q + 1)
    assert np.array_equal(bits(im[q - i + 1]), bits(re[i - 1]))          # :64-66
    assert np.array_equal(bits(re[i + q]), bits(-re[q - i])) and np.array_equal(bits(im[i + q]), bits(im[q - i]))
    assert np.array_equal(bits(re[i + 2 * q]), bits(-re[i])) and np.array_equal(bits(im[i + 2 * q]), bits(-im[i]))
    i = i[:-1]  # (:74 overwrites the last entry of the fourth quarter with roots[0])
    assert np.array_equal(bits(re[i + 3 * q]), bits(re[q - i])) and np.array_equal(bits(im[i + 3 * q]), bits(-im[q - i]))
    # each first-quarter cosine within one ulp of the true cosine of the argument the reference forms
    mpmath.mp.dps = 60
    angle = 2 * 3.141592653589793 / float(M)
    for k in range(q):
        x = angle * float(k)
        true = mpmath.cos(mpmath.mpf(x))
        assert abs(mpmath.mpf(float(re[k])) - true) <= mpmath.mpf(math.ulp(float(re[k]))), k


# ---- the quantiser -----------------------------------------------------------------------------------------------------------------
PRIMES = {30: downstream_primes(30, 64, 1)[0], 45: downstream_primes(45, 64, 1)[0], 61: downstream_primes(61, 64, 1)[0]}


def check_word_against_the_rule(w, value, scale, q):
    """the rule as properties of the word, in exact rationals: which integer it stands for, its residue class and its range"""
    if value == 0:
        assert w == 0
        return
    v = Fraction(abs(float(value) * float(scale)))  # the float64 product, exactly
    if v >= 2 ** 64:
        assert v.denominator == 1  # the integer is v itself: v + 1/2 is no float64 there and rounds back to v
        I = int(v)
    else:
        t = Fraction(float(v) + 0.5)  # the float64 sum, exactly (it is v + 1/2 unless that is no float64)
        I = t.numerator // t.denominator
        assert abs(Fraction(I) - v) <= Fraction(1, 2) + Fraction(1, 2 ** 53) or v >= 2 ** 52  # the nearest integer, halves up
    if value < 0:
        # -I mod q in (0, q]: q stands for the residue 0 -- except at I == q exactly, which is not `c > q` and gives q - c = 0
        assert (w + I) % q == 0 and 0 <= w <= q and (w == 0) == (I == q), (value, scale, w)
    elif v < 2 ** 64 and I <= 0x1FFFFFFFFFFFFFFF:
        assert w == I, (value, scale, w)  # unreduced, even at or above q
    else:
        assert (w - I) % q == 0 and 0 <= w < q, (value, scale, w)


@pytest.mark.parametrize("bits", [30, 45, 61])
def test_quantiser_edge_list(bits):
    q = PRIMES[bits]
    seen, cs = set(), set()
    for value, scale in R.quantiser_cases(q):
        w = R.quantise_word(value, scale, q)
        check_word_against_the_rule(w, value, scale, q)
        seen.add("q" if w == q else "big" if w > q else "zero" if w == 0 else "canonical")
        v = abs(value * scale)
        if v < 2.0 ** 64:
            cs.add(int(v + 0.5))
    assert {"q", "zero", "canonical"} <= seen and (bits == 61 or "big" in seen), seen
    # the list reaches both sides of `c > q`, and c = q itself where q is a float64
    assert any(c > q for c in cs) and any(0 < c < q for c in cs) and (bits == 61 or q in cs)
    assert R.quantise_word(0.49999999999999994, 1.0, q) == 1 and R.quantise_word(-0.49999999999999994, 1.0, q) == q - 1
    assert R.quantise_word(-0.25, 1.0, q) == q            # c = 0 of a non-zero negative value: the word q
    assert R.quantise_word(-1.0, 0.0, q) == q and R.quantise_word(1.0, 0.0, q) == 0 and R.quantise_word(-1e-300, 1e-30, q) == q
    if bits <= 53:
        assert R.quantise_word(-float(q), 1.0, q) == 0 and R.quantise_word(-float(q + 1), 1.0, q) == q - 1  # c == q is not c > q
        assert R.quantise_word(-float(2 * q), 1.0, q) == q and R.quantise_word(-float(q) * 2.0 ** 64, 1.0, q) == q


@pytest.mark.parametrize("ci", [False, True])
@pytest.mark.parametrize("bits", [30, 45, 61])
def test_quirk_words_through_the_oracles_transform(bits, ci):
    """the strict NTT of the quantiser's words equals the NTT of their residues: what lets the device reduce first"""
    N = 16
    q = downstream_primes(bits, 4 * N, 1)[0]
    ring = O.Ring(N, [q], ci)
    words = [R.quantise_word(v, s, q) for v, s in R.quantiser_cases(q)]
    for at in range(0, len(words), N):
        chunk = (words[at: at + N] + [0] * N)[:N]
        x = np.array([chunk], dtype=np.uint64)
        red = np.array([[w % q for w in chunk]], dtype=np.uint64)
        assert np.array_equal(ring.NTT(x), ring.NTT(red)), (bits, at)
        assert np.array_equal(ring.unop("MForm", x), ring.unop("MForm", red)), (bits, at)


# ---- reconstruction -----------------------------------------------------------------------------------------------------------------
def rne_statement(x: int) -> float:
    """round to nearest, ties to even, of an integer to 53 bits, by hand"""
    if x == 0:
        return 0.0
    a, s = abs(x), (-1.0 if x < 0 else 1.0)
    sh = max(a.bit_length() - 53, 0)
    m, rem = a >> sh, a & ((1 << sh) - 1)
    half = 1 << (sh - 1) if sh else 0
    if sh and (rem > half or (rem == half and (m & 1))):
        m += 1
    try:
        return s * math.ldexp(float(m), sh)
    except OverflowError:  # beyond the float64 range (32 limbs of 55 bits): Float64() returns the infinity
        return s * math.inf


@pytest.mark.parametrize("nlimbs", [2, 32])
def test_reconstruction_edge_list(nlimbs):
    moduli = downstream_primes(55, 64, nlimbs)
    Q = math.prod(moduli)
    scale = 2.0 ** 20
    for x in R.reconstruction_cases(Q):
        res = [x % q for q in moduli]
        c = x % Q
        c = c - Q if c >= Q >> 1 else c
        assert R.coeff_to_float(res, moduli, scale) == rne_statement(c) / scale, x
    assert R.coeff_to_float([(2 ** 100 + 2 ** 47) % q for q in moduli], moduli, 1.0) == 2.0 ** 100               # the tie goes to even
    assert R.coeff_to_float([(2 ** 100 + 2 ** 47 + 1) % q for q in moduli], moduli, 1.0) == 2.0 ** 100 + 2.0 ** 48  # the sticky bit decides
    assert R.coeff_to_float([(Q >> 1) % q for q in moduli], moduli, 1.0) < 0 < R.coeff_to_float([((Q >> 1) - 1) % q for q in moduli], moduli, 1.0)


def test_one_limb_reconstruction_is_the_no_crt_formula():
    q = PRIMES[61]
    for c in (0, 1, (q >> 1) - 1, q >> 1, q - 1, 2 ** 53 + 1, q - 2 ** 53 - 1):
        want = -float(q - c) if c >= q >> 1 else float(c)  # polyToFloatNoCRT (encoder.go:1141-1147)
        assert R.coeff_to_float([c], [q], 8.0) == want / 8.0


# ---- encode -> decode ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [False, True])
@pytest.mark.parametrize("logN,log_slots,log_scale", [(6, 5, 45), (8, 7, 30), (8, 3, 45)])
def test_restated_round_trip_within_the_reference_bound(logN, log_slots, log_scale, ci):
    """schemes/ckks/ckks_test.go:278-283: log2(1 / err) >= log2(scale) - (logN + 2)"""
    N = 1 << logN
    M = (4 if ci else 2) * N
    if ci:
        log_slots += 1
    moduli = downstream_primes(55, 2 * M, 2)
    rre, rim = lib_roots(M)
    rng = rng_for(4300 + logN)
    slots = 1 << log_slots
    z = rng.uniform(-1, 1, slots) + (0 if ci else 1j * rng.uniform(-1, 1, slots))
    coeffs = R.embed_coeffs(z, log_slots, N, ci, M, rre, rim)
    words = R.quantise_poly(coeffs, 2.0 ** log_scale, moduli, N)
    re, im = R.decode_slots(words, moduli, 2.0 ** log_scale, log_slots, N, ci, M, rre, rim)
    err = max(np.max(np.abs(re - z.real)), np.max(np.abs(im - z.imag)))
    assert math.log2(1 / err) >= log_scale - (logN + 2), (err, log_scale)


# ---- the header, the recorder and the mirrors ------------------------------------------------------------------------------------
def test_header_symbols_declared_and_exported():
    syms = _lib.declared_symbols()
    for s in NEW:
        assert s in syms, s
    assert os.path.exists(_lib.lib_path()), "libhering.so not built"
    L = _lib.load()
    missing = [s for s in NEW if not hasattr(L, s)]
    assert not missing, missing
    # host data: no replay numbers -- the numbered tables end where they did, at 72
    tables = (_lib._TRACE_FNS, _lib._TRACE_FNS_RGSW, _lib._TRACE_FNS_BLINDROT, _lib._TRACE_FNS_BRIDGE, _lib._TRACE_FNS_BFV)
    assert max(v[0] for t in tables for v in t.values()) == 72
    assert not any(s in t for s in NEW for t in tables)
    for s in ("he_ckks_decode", "he_ckks_fft", "he_ckks_ifft", "he_ckks_roots_host", "he_ckks_encoder_roots", "he_ckks_encoder_info",
              "he_ckks_encoder_destroy"):
        assert s in _lib._TRACE_IGNORE, s
    assert "he_ckks_encode" not in _lib._TRACE_IGNORE and "he_ckks_encode_qp" not in _lib._TRACE_IGNORE
    names = [L.he_prof_kernel_name(i).decode() for i in range(64)]
    for k in ("special_fft", "ckks_fft_pass", "special_ifft_quantize", "f64_to_rns", "rns_to_f64"):
        assert k in names, k


def test_header_states_its_scope_and_differences():
    text = open(HEADER).read()
    for phrase in ("Out of scope", "embedArbitrary", "non-finite inputs", "math.Cos", "32 limbs", "no fused multiply-add", "0x1fffffffffffffff"):
        assert phrase in text, phrase
    assert '#include "hering.h"' in text
    assert "he_ckks_enc" not in open(os.path.join(ROOT, "include", "hering.h")).read()


def test_roots_host_rejects_bad_orders():
    L = _lib.load()
    buf = np.zeros(64)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert L.he_ckks_roots_host(24, p) != 0 and L.he_ckks_roots_host(4, p) != 0 and L.he_ckks_roots_host(16, None) != 0
    assert L.he_ckks_roots_host(16, p) == 0 and buf[0] == 1.0 and buf[32] == 1.0


def test_check_go_abi_reports_the_encoder_file():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_go_abi.py")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ckks.Encoder" in out.stdout
    src = open(os.path.join(ROOT, "go", "hering", "encoder.go")).read()
    for s in NEW:
        assert re.search(r"C\." + s + r"\(", src), s


def test_cpp_mirror_compiles_with_the_encoder():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "ckks_encoder_mirror.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
