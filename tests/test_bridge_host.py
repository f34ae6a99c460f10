"""The CKKS bridge on the host (no GPU): the closed form of the fold's index table, the two coefficient-domain identities the maps
stand for, the reference's DomainSwitcher sequences (tests/bridge_ref.py) against the scheme with real keys, and the new header's
symbols, aliasing rows and mirrors.

The maps (ring/conjugate_invariant.go:3-44), N = 2n, both rings over the same moduli q = 1 mod 2N:
    fold:    INTT_CI(Fold(NTT_std(a)))   = (2 a_0, a_1 - a_{N-1}, ..., a_{n-1} - a_{n+1})          (a + a(X^-1), compressed)
    unfold:  INTT_std(Unfold(NTT_CI(c))) = (c_0, c_1, ..., c_{n-1}, 0, -c_{n-1}, ..., -c_1)        (c_j (X^j + X^-j), X^-j = -X^{N-j})
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from lattigo_amd import _lib
from oracle import oracle as O
from tests import bridge_aliasing as BA
from tests import bridge_ref as B
from tests.helpers import rng_for, uniform_poly
from tests.rlwe_fixtures import SecretKey

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hering_bridge.h")
NEW = ("he_unfold_conjugate_invariant_to_standard", "he_fold_standard_to_conjugate_invariant", "he_complex_to_real", "he_real_to_complex")


# ---- the index table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logN", range(4, 17))
def test_fold_index_table_is_the_mirror(logN):
    """AutomorphismNTTIndex(N, 2N, 2N-1)[i] = i XOR (N-1) = N-1-i: the device kernels take no table"""
    N = 1 << logN
    idx = B.fold_index(N)
    i = np.arange(N, dtype=np.uint64)
    assert np.array_equal(idx, i ^ np.uint64(N - 1))
    assert np.array_equal(idx, np.uint64(N - 1) - i)


# ---- the coefficient-domain identities ------------------------------------------------------------------------------------------
def _signed_sub(a, b, q):
    """(a - b) mod q limb-wise on uint64 rows below q"""
    qi = np.array(q, dtype=np.uint64)[:, None]
    return np.where(a >= b, a - b, a + qi - b)


def fold_coeff(a, q):
    """[limbs, N] coefficients -> (2 a_0, a_j - a_{N-j}) mod q, [limbs, N/2]"""
    N = a.shape[1]
    n = N // 2
    out = np.empty((a.shape[0], n), dtype=np.uint64)
    out[:, 1:] = _signed_sub(a[:, 1:n], a[:, :n:-1], q)
    for i, qi in enumerate(q):
        out[i, 0] = 2 * int(a[i, 0]) % int(qi)
    return out


def unfold_coeff(c, q):
    """[limbs, n] coefficients -> (c_j at j < n, 0 at n, -c_j at N - j), [limbs, 2n]"""
    n = c.shape[1]
    out = np.zeros((c.shape[0], 2 * n), dtype=np.uint64)
    out[:, :n] = c
    qi = np.array(q, dtype=np.uint64)[:, None]
    neg = np.where(c == 0, c, qi - c)
    out[:, n + 1:] = neg[:, :0:-1]
    return out


Q3, _ = O.GenModuli(13, [45, 58, 61], [])  # = 1 mod 2^13: both ring types up to a standard degree of 2^12
Q3 = list(Q3)


@pytest.mark.parametrize("logN", range(5, 13))
def test_fold_and_unfold_identities_and_round_trip(logN):
    N, n = 1 << logN, 1 << (logN - 1)
    std, ci = O.Ring(N, Q3), O.Ring(n, Q3, True)
    rng = rng_for(8000 + logN)
    top = lambda m: np.array([[qi - 1] * m for qi in Q3], dtype=np.uint64)  # every word q - 1: the largest sums
    for x in (uniform_poly(rng, Q3, N), top(N)):  # NTT-domain words of the standard ring
        assert np.array_equal(ci.INTT(B.fold(x, Q3)), fold_coeff(std.INTT(x), Q3)), ("fold", logN)
    for y in (uniform_poly(rng, Q3, n), top(n)):  # NTT-domain words of the conjugate-invariant ring
        assert np.array_equal(std.INTT(B.unfold(y)), unfold_coeff(ci.INTT(y), Q3)), ("unfold", logN)
        # round trip: Fold(Unfold(y)) = 2 y mod q
        assert np.array_equal(B.fold(B.unfold(y), Q3), ci.binop("Add", y, y)), ("round trip", logN)


def test_fold_wraps_lazy_words_as_the_reference():
    """words at or above q: the 64-bit sum wraps, then one conditional subtraction (SubRing.Add on lazy words)"""
    q = Q3[2]
    a = np.array([[2**64 - 1, q, q + 5, 7] + [0] * 28], dtype=np.uint64)
    a[0, 31], a[0, 30], a[0, 29], a[0, 28] = 3, 2**64 - q, q - 1, 2**63
    out = B.fold(a, [q])
    want = [(2**64 - 1 + 3) % 2**64, (q + 2**64 - q) % 2**64, (q + 5 + q - 1) % 2**64, (7 + 2**63) % 2**64]
    want = [w - q if w >= q else w for w in want]
    assert [int(x) for x in out[0, :4]] == want


# ---- the scheme: real keys --------------------------------------------------------------------------------------------------------
LOGN, EBOUND = 10, B.EBOUND


@pytest.mark.parametrize("n_special", [1, 2])
def test_domain_switcher_with_real_keys(n_special):
    """N = 2^10, three 55-bit moduli, one or two 61-bit special primes; fresh errors and key errors |e| <= EBOUND = 19.

    The noise bound, coefficient-wise and worst case, on the centred phase:
      KS, one key switch at degree N: the gadget product's sum over `digits` digits of a negacyclic product of a digit (below
        dmax: the product of the digit's moduli) with a key error (below EBOUND), divided by P: digits N dmax EBOUND / P + 1;
        plus ModDown's division by P on both components, at most 1 per coefficient each (the centred remainder's 1/2 and the
        basis extension's unit), component 1 against a ternary secret of N coefficients: 1 + N.
      RealToComplex: the unfold is the ring embedding (exact: the mapped key is the unfold of the real key), so the phase under
        skStd is Unfold(m + e) + e_KS: |.| <= E1 = EBOUND + KS.
      ComplexToReal: the key switch to the mapped key, which the fold's automorphism X -> X^-1 fixes, then a + a(X^-1) on the
        phase, two coefficients per output (2 a_0 at 0): |.| <= 2 (EBOUND + KS) on a fresh ciphertext.
      The frame of EvaluateConjugateInvariant: A + i B carries 2 E1, ComplexToReal folds it (4 E1) and adds its own folded key
        switch (2 KS); the multiplication by -i permutes coefficients up to sign: each output within 4 E1 + 2 KS of 2 m."""
    N, n = 1 << LOGN, 1 << (LOGN - 1)
    q, p = O.GenModuli(LOGN + 1, [55] * 3, [61] * n_special)
    q, p = list(q), list(p)
    oQ, oP, ciQ = O.Ring(N, q), O.Ring(N, p), O.Ring(n, q, True)
    oev = O.Evaluator(oQ, oP)
    rng = rng_for(8100 + n_special)
    sk_std = SecretKey(rng, oQ, oP)
    sk_ci, sk_map, k_c2r, k_r2c = B.gen_ring_swap_keys(rng, oQ, oP, sk_std, rng.integers(-1, 2, size=n))
    level = len(q) - 1
    KS = B.key_switch_noise_bound(N, q, p)
    E1 = EBOUND + KS
    worst = lambda got, want: max(abs(int(g) - int(w)) for g, w in zip(got, want))

    # RealToComplex of an encryption of m under skCI: the phase under skStd is Unfold(m)
    m = rng.integers(-(1 << 30), 1 << 30, size=n)
    ct = B.encrypt(rng, ciQ, sk_ci.Q, m)
    up = B.real_to_complex(oev, oQ, level, ct, k_r2c)
    e = worst(B.centred_phase(oQ, up, sk_std.Q), B.unfold_ints(m))
    print(f"RealToComplex: noise {e}, bound {E1}")
    assert e <= E1
    # ComplexToReal of an encryption of M under skStd: the phase under skCI is the folded M
    M = rng.integers(-(1 << 30), 1 << 30, size=N)
    ctM = B.encrypt(rng, oQ, sk_std.Q, M)
    down = B.complex_to_real(oev, oQ, level, ctM, k_c2r)
    e = worst(B.centred_phase(ciQ, down, sk_ci.Q), B.fold_ints(M))
    print(f"ComplexToReal: noise {e}, bound {2 * (EBOUND + KS)}")
    assert e <= 2 * (EBOUND + KS)

    # the frame of bootstrapping.Evaluator.EvaluateConjugateInvariant (evaluator.go:460-508) without the bootstrap
    ma, mb = rng.integers(-(1 << 30), 1 << 30, size=n), rng.integers(-(1 << 30), 1 << 30, size=n)
    cta, ctb = B.encrypt(rng, ciQ, sk_ci.Q, ma), B.encrypt(rng, ciQ, sk_ci.Q, mb)
    A, Bc = B.real_to_complex(oev, oQ, level, cta, k_r2c), B.real_to_complex(oev, oQ, level, ctb, k_r2c)
    mono = B.monomial_i(oQ)
    mul = lambda c, x: np.stack([oQ.binop("MulCoeffsMontgomery", c[k], x) for k in range(2)])
    Cc = np.stack([oQ.binop("Add", A[k], mul(Bc, mono)[k]) for k in range(2)])  # A + i B
    out_a = B.complex_to_real(oev, oQ, level, Cc, k_c2r)
    out_b = B.complex_to_real(oev, oQ, level, mul(Cc, oQ.unop("Neg", mono)), k_c2r)  # (-i) (A + i B) = B - i A
    bound = 4 * E1 + 2 * KS
    for name, out, msg in (("real part", out_a, ma), ("imaginary part", out_b, mb)):
        e = worst(B.centred_phase(ciQ, out, sk_ci.Q), [2 * int(x) for x in msg])
        print(f"frame, {name}: noise {e}, bound {bound}")
        assert e <= bound


# ---- the header, the recorder and the mirrors ------------------------------------------------------------------------------------
def test_header_symbols_declared_and_exported():
    syms = _lib.declared_symbols()
    for s in NEW:
        assert s in syms, s
    assert os.path.exists(_lib.lib_path()), "libhering.so not built"
    L = _lib.load()
    missing = [s for s in NEW if not hasattr(L, s)]
    assert not missing, missing
    # replayable: the recorder knows every new entry, numbered on from the last existing one in a table of its own
    last = max(v[0] for t in (_lib._TRACE_FNS, _lib._TRACE_FNS_RGSW, _lib._TRACE_FNS_BLINDROT) for v in t.values())
    assert sorted(_lib._TRACE_FNS_BRIDGE[s][0] for s in NEW) == list(range(last + 1, last + 5))
    names = [L.he_prof_kernel_name(i).decode() for i in range(64)]
    assert "ci_bridge_fold" in names and "ci_bridge_unfold" in names
    assert names.index("ci_bridge_unfold") == names.index("ci_bridge_fold") + 1 == names.index("automorphism_ct_select") + 2


def test_aliasing_rows_are_the_header_entry_points():
    from tests.test_aliasing_table import poly_entries
    entries = poly_entries(open(HEADER).read())
    assert sorted(entries) == sorted(BA.ROWS)
    for name, params in entries.items():
        assert list(BA.ROWS[name].params) == params, (name, params)
    for name in ("he_complex_to_real", "he_real_to_complex"):
        r = BA.ROWS[name]
        assert r.verdict("out0", "out1") == "reject" and r.verdict("in0", "in1") == "accept"
        assert all(r.verdict(o, i) == "reject" for o in ("out0", "out1") for i in ("in0", "in1"))


def test_check_go_abi_reports_the_domain_switcher():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_go_abi.py")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ckks.DomainSwitcher: ComplexToReal, RealToComplex" in out.stdout
    src = open(os.path.join(ROOT, "go", "hering", "bridge.go")).read()
    assert re.search(r"C\.he_complex_to_real\(", src) and re.search(r"C\.he_real_to_complex\(", src)


def test_python_mirror_reports_a_missing_key_as_the_reference():
    from lattigo_amd import bridge

    class _P:  # (no device: the key check comes before any call of the library)
        h = 0

        def Level(self):
            return 0
    sw = bridge.DomainSwitcher(_P(), None, None)
    with pytest.raises(_lib.HeringError, match="cannot ComplexToReal: no realToComplexEvk provided"):
        sw.ComplexToReal([_P(), _P()], [_P(), _P()])
    with pytest.raises(_lib.HeringError, match="cannot RealToComplex: no realToComplexEvk provided"):
        sw.RealToComplex([_P(), _P()], [_P(), _P()])


def test_cpp_mirror_compiles_with_the_bridge():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "bridge_mirror.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
