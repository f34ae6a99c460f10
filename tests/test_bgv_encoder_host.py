"""The restatement of the reference's bgv.Encoder (tests/bgv_encoder_ref.py) against definitions that do not share its code: the
index matrix against its closed form, the encoding against the ring structure it promises (slot-wise products, row rotations), the
two ring maps against big-integer statements, the int64 path against plain Python arithmetic, and the wiring of
include/hering_bgv_encoder.h.  No GPU."""
import os

import numpy as np
import pytest

from lattigo_amd import _lib
from tests import bgv_encoder_ref as R
from tests.helpers import prod, rng_for, uniform_poly
from tests.rlwe_fixtures import downstream_primes, negacyclic_mul_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["he_bgv_encoder_create", "he_bgv_encoder_destroy", "he_bgv_encoder_info", "he_bgv_encoder_index", "he_bgv_encode_ring_t",
       "he_bgv_decode_ring_t", "he_bgv_ring_t2q", "he_bgv_ring_q2t", "he_bgv_encode", "he_bgv_encode_qp", "he_bgv_decode"]
T60 = downstream_primes(60, 1 << 14, 1)[0]
_P = {}


def params(logN, nq, T):
    if (logN, nq, T) not in _P:
        _P[(logN, nq, T)] = R.Params(logN, downstream_primes(55, 2 << logN, nq), T)
    return _P[(logN, nq, T)]


@pytest.mark.parametrize("logN", [4, 7, 10])
def test_permute_matrix_closed_form(logN):
    """slot i of row r sits where the bit-reversed transform puts the evaluation at psi^(+-5^i): index bitrev(((+-5^i mod 2N) - 1) / 2)"""
    N = 1 << logN
    perm = R.permute_matrix(logN)
    assert sorted(int(x) for x in perm) == list(range(N))
    for i in range(N >> 1):
        e = pow(5, i, 2 * N)
        assert int(perm[i]) == R.bit_reverse((e - 1) >> 1, logN) and int(perm[i + (N >> 1)]) == R.bit_reverse((2 * N - e - 1) >> 1, logN)


def test_log_nt_is_the_rule_of_new_parameters():
    assert [R.log_nt(10, T) for T in (97, 257, 12289, 65537, 65929217)] == [4, 7, 10, 10, 10]
    assert R.log_nt(16, 65537) == 15 and R.log_nt(12, 12289) == 11


@pytest.mark.parametrize("T", [97, 257, 65537, T60])
def test_decode_of_encode(T):
    P = params(10, 3, T)
    rng = rng_for(6400 + T % 1000)
    for n in (1, P.NT - 1, P.NT):
        v = rng.integers(0, T, n, dtype=np.uint64)
        s = rng.integers(-(T >> 1) - 1, T >> 1, n).astype(np.int64)
        for ntt, mont, scale in ((True, False, 1), (False, False, T - 1), (True, True, int(rng.integers(1, T)))):
            w = P.embed(v, scale, 2, ntt, mont, True, False)
            if mont:
                w = P.oQ.unop("IMForm", w)
            assert np.array_equal(P.decode(w, scale, 2, True, ntt, False)[:n], v) and not P.decode(w, scale, 2, True, ntt, False)[n:].any()
            w = P.embed(s, scale, 2, ntt, False, True, True)
            assert np.array_equal(P.decode(w, scale, 2, True, ntt, True)[:n], s)
    if P.gap == 1:
        v = rng.integers(0, T, P.N - 3, dtype=np.uint64)
        w = P.encode_coeffs(v, 5, 2, True, False)
        assert np.array_equal(P.decode(w, 5, 2, False, True, False)[: P.N - 3], v)


@pytest.mark.parametrize("T", [257, 65537])
def test_ring_structure(T):
    """the negacyclic product modulo T of two encodings decodes to the slot-wise product; X -> X^5 rotates each row by one;
    X -> X^(2N - 1) swaps the rows"""
    P = params(10, 2, T)
    n, h = P.NT, P.NT >> 1
    rng = rng_for(6500 + T % 1000)
    a, b = rng.integers(0, T, (2, n), dtype=np.uint64)
    pa, pb = P.encode_ring_t(a, 1, False)[0], P.encode_ring_t(b, 1, False)[0]
    pc = negacyclic_mul_mod([int(x) for x in pa], [int(x) for x in pb], T).astype(np.uint64)
    assert np.array_equal(P.decode_ring_t(pc, 1, False), np.array([int(x) * int(y) % T for x, y in zip(a, b)], dtype=np.uint64))

    def automorphism(p, g):
        out = np.zeros(n, dtype=np.uint64)
        for i in range(n):
            e = i * g % (2 * n)
            out[e % n] = (T - int(p[i])) % T if e >= n else p[i]
        return out

    rot = P.decode_ring_t(automorphism(pa, 5), 1, False)
    assert np.array_equal(rot[:h], np.roll(a[:h], -1)) and np.array_equal(rot[h:], np.roll(a[h:], -1))
    swap = P.decode_ring_t(automorphism(pa, 2 * n - 1), 1, False)
    assert np.array_equal(swap[:h], a[h:]) and np.array_equal(swap[h:], a[:h])


@pytest.mark.parametrize("T,logN", [(65537, 10), (257, 10), (12289, 12), (T60, 10)])
def test_ring_maps(T, logN):
    """RingQ2T(RingT2Q(p)) == p; RingQ2T against the centred big-integer value on random words and on the edge list.  The two
    level > 0 branches differ next to Q >> 1, as they do in the reference: with gap 1, x = (Q >> 1) - 1 makes x + Q/2 = Q - 2, the
    float sum of reconstructRNS lands within an ulp of an integer, v comes out one too large and the word is that of x - Q
    (asserted as such, against the oracle's own ModUpQtoP); with gap > 1 the reconstruction is exact.  At x = Q >> 1 itself the
    same rounding gives x - Q, which is also what the centring x >= Q >> 1 -> x - Q of PolyToBigintCentered gives: there the two
    agree."""
    P = params(logN, 3, T)
    rng = rng_for(6600 + T % 1000)
    p = rng.integers(0, T, (1, P.NT), dtype=np.uint64)
    for level, scaled in ((0, False), (0, True), (2, False), (2, True)):
        if prod(P.q[: level + 1]) > 2 * T:  # (a round trip needs T to fit the centred range of Q)
            assert np.array_equal(P.ring_q2t(P.ring_t2q(p, level, scaled), level, scaled), p), (level, scaled)
    for level in (1, 2):
        mods = P.q[: level + 1]
        Q = prod(mods)
        w = uniform_poly(rng, mods, P.N)
        edge = [0, 1, T % Q, Q - 1, (Q >> 1) + 1, (Q >> 1) - 1]
        for k, x in enumerate(edge):
            w[:, k * P.gap] = R.words_of(x, mods)
        got = P.ring_q2t(w, level, False)[0]
        want = np.array([R.centred_value(w[:, j], mods) % T for j in range(0, P.N, P.gap)], dtype=np.uint64)
        if P.gap == 1:
            assert int(got[5]) == ((Q >> 1) - 1 - Q) % T == int(P.be.ModUpQtoP(level, 0, w)[0][5]) % T and got[5] != want[5]
            want[5] = got[5]
        assert np.array_equal(got, want), level
        # x = Q >> 1 on its own
        w[:, 0] = R.words_of(Q >> 1, mods)
        got = int(P.ring_q2t(w, level, False)[0][0])
        assert got == ((Q >> 1) - Q) % T
        if P.gap == 1:
            assert got == int(P.be.ModUpQtoP(level, 0, w)[0][0]) % T


def test_int64_edges():
    for T in (97, 65537, T60):
        edges = [0, 1, -1, T - 1, -(T - 1), T, -T, T + 1, -(T + 1), -2 * T, (1 << 63) - 1, -(1 << 63)]
        got = R.reduce_words(np.array(edges, dtype=np.int64), T, True)
        for c, w in zip(edges, got):
            assert w % T == c % T and (w == T) == (c < 0 and c % T == 0), (T, c, w)  # the reference's word T for a negative multiple of T
        u = [0, 1, T - 1, T, T + 1, 1 << 63, (1 << 64) - 1]
        assert R.reduce_words(np.array(u, dtype=np.uint64), T, False) == [x % T for x in u]
    P = params(10, 2, 257)
    s = np.array([-129, -128, -1, 0, 127], dtype=np.int64)  # centred range: value >= T >> 1 -> value - T
    assert np.array_equal(P.centre(np.array([x % 257 for x in map(int, s)], dtype=np.uint64), True), s)


def test_header_is_wired():
    syms = _lib.declared_symbols()
    assert all(s in syms for s in NEW)
    L = _lib.load()
    assert all(hasattr(L, s) and getattr(L, s).argtypes is not None for s in NEW)
    for s in ("he_bgv_decode", "he_bgv_decode_ring_t", "he_bgv_encoder_info", "he_bgv_encoder_index", "he_bgv_encoder_destroy"):
        assert s in _lib._TRACE_IGNORE
    for s in ("he_bgv_encode", "he_bgv_encode_qp", "he_bgv_encode_ring_t", "he_bgv_ring_t2q", "he_bgv_ring_q2t"):
        assert s not in _lib._TRACE_IGNORE
    assert "he_bgv_enc" not in open(os.path.join(ROOT, "include", "hering.h")).read()
