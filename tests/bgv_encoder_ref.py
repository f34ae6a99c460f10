"""Restatement of the reference's bgv.Encoder (schemes/bgv/encoder.go) in Python integers and numpy over the oracle, for the tests of
include/hering_bgv_encoder.h: oracle.Ring(N_T, [T]) for the transforms modulo T, oracle.BasisExtender(ringQ, ringT).ModUpQtoP for
the gap-1, level > 0 branch of RingQ2T (the same AddScalarBigint / ModUpExact / SubScalarBigint sequence with the same constants,
its words reduced modulo T), Python big integers for PolyToBigintCentered.

Where the header states a deliberate difference the restatement follows the header: RingT2Q writes canonical words, its scale_up
on a polynomial of ringP multiplies by T^-1 mod p_j, RingQ2T returns canonical words.  Everything else is the reference line by
line; one polynomial per call, [limbs][N] uint64.  A plain helper module (not a conftest)."""
from __future__ import annotations

import functools

import numpy as np

from oracle import oracle as O
from tests.helpers import prod

M64 = (1 << 64) - 1
GALOIS_GEN = 5


def bit_reverse(x: int, bits: int) -> int:
    r = 0
    for _ in range(bits):
        r = (r << 1) | (x & 1)
        x >>= 1
    return r


def permute_matrix(logN: int) -> np.ndarray:
    """permuteMatrix (:110-133)"""
    N = 1 << logN
    mask, pw = 2 * N - 1, 1
    perm = np.zeros(N, dtype=np.uint64)
    for i in range(N >> 1):
        pos = bit_reverse(pw >> 1, logN)
        perm[i], perm[i + (N >> 1)] = pos, N - pos - 1
        pw = (pw * GALOIS_GEN) & mask
    return perm


def log_nt(logN: int, T: int) -> int:
    """schemes/bgv/params.go:120-123: the largest ring of degree at most N in which T = 1 mod 2 N_T"""
    v2 = ((T - 1) & -(T - 1)).bit_length() - 1
    return min(logN, v2 - 1)


def reduce_words(values, T: int, signed: bool):
    """the words EncodeRingT / Encode place (:220-224, :237-244): unsigned -- BRedAdd(v); int64 -- sign = c >> 63,
    abs = BRedAdd(uint64(c * (1 - 2 sign))) in wrapping arithmetic, the word abs or T - abs (T for a negative multiple of T)"""
    out = []
    for v in np.asarray(values).reshape(-1):
        u = int(v) & M64
        if not signed:
            out.append(u % T)
            continue
        sign = u >> 63
        a = ((-u) & M64 if sign else u) % T
        out.append(T - a if sign else a)
    return out


class Params:
    """the rings of one parameter set in the oracle: Q (and P) of degree N = 2^logN, ringT of degree N_T, the index matrix"""

    def __init__(self, logN: int, q, T: int, p=()):
        self.logN, self.N, self.q, self.p, self.T = logN, 1 << logN, [int(x) for x in q], [int(x) for x in p], int(T)
        self.logNT = log_nt(logN, self.T)
        self.NT, self.gap = 1 << self.logNT, 1 << (logN - self.logNT)
        self.oQ, self.oT = O.Ring(self.N, self.q), O.Ring(self.NT, [self.T])
        self.oP = O.Ring(self.N, self.p) if self.p else None
        self.be = O.BasisExtender(self.oQ, self.oT) if self.gap == 1 and len(self.q) > 1 else None
        self.perm = permute_matrix(self.logNT)

    # ---- ring T ---------------------------------------------------------------------------------------------------------------
    def mul_scalar_t(self, pT, s: int):
        return self.oT.scalarop("MulScalar", np.asarray(pT, dtype=np.uint64).reshape(1, self.NT), int(s))

    def encode_ring_t(self, values, scale: int, signed: bool) -> np.ndarray:
        """EncodeRingT (:203-262): [1][N_T]"""
        pt = np.zeros((1, self.NT), dtype=np.uint64)  # (:252-255: the unmapped slots are zeroed)
        for i, w in enumerate(reduce_words(values, self.T, signed)):
            pt[0, int(self.perm[i])] = w
        return self.mul_scalar_t(self.oT.INTT(pt), scale)

    def centre(self, words, signed: bool) -> np.ndarray:
        """:356-368"""
        w = np.asarray(words, dtype=np.uint64).reshape(-1)
        if not signed:
            return w.copy()
        half = self.T >> 1
        return np.array([int(x) - self.T if int(x) >= half else int(x) for x in w], dtype=np.int64)

    def decode_ring_t(self, pT, scale: int, signed: bool) -> np.ndarray:
        """DecodeRingT (:341-374): [N_T]"""
        tmp = self.oT.NTT(self.mul_scalar_t(pT, pow(int(scale), self.T - 2, self.T)))
        return self.centre(tmp[0][self.perm.astype(np.int64)], signed)

    # ---- ring T <-> RNS -------------------------------------------------------------------------------------------------------
    def ring_t2q(self, pT, level: int, scale_up: bool, to_p: bool = False) -> np.ndarray:
        """RingT2Q (:378-407), canonical words: [level + 1][N]"""
        mods = (self.p if to_p else self.q)[: level + 1]
        c = [int(x) for x in np.asarray(pT).reshape(-1)]
        out = np.zeros((level + 1, self.N), dtype=np.uint64)
        for i, qi in enumerate(mods):
            k = pow(self.T, -1, qi) if scale_up else 1
            out[i, :: self.gap] = np.array([x * k % qi for x in c], dtype=np.uint64)
        return out

    def ring_q2t(self, pQ, level: int, scale_down: bool) -> np.ndarray:
        """RingQ2T (:412-467), canonical words: [1][N_T]"""
        mods, T = self.q[: level + 1], self.T
        poly = np.asarray(pQ, dtype=np.uint64)[: level + 1]
        if scale_down:  # :423
            poly = self.oQ.scalarop("MulScalar", poly, T, level=level)
        if level == 0:  # :447-465
            q = mods[0]
            out = []
            for v in poly[0, :: self.gap]:
                x = (int(v) + (q >> 1)) & M64
                x = x - q if x >= q else x                      # AddScalar
                out.append((x % T + T - (q >> 1) % T) % T)      # Reduce, SubScalar
            return np.array([out], dtype=np.uint64)
        if self.gap == 1:  # :434-436
            up = self.be.ModUpQtoP(level, 0, poly)  # (the oracle's ModUpQtoP is that whole sequence, ring/basis_extension.go:178-193)
            return np.array([[int(x) % T for x in up[0]]], dtype=np.uint64)
        return np.array([[centred_value(poly[:, j], mods) % T for j in range(0, self.N, self.gap)]], dtype=np.uint64)  # :438-440

    # ---- Encode / Decode ------------------------------------------------------------------------------------------------------
    def _finish(self, w, to_p, level, ntt, mont):
        ring = self.oP if to_p else self.oQ
        if ntt:
            w = ring.NTT(w, level=level)
        if mont:
            w = ring.unop("MForm", w, level=level)
        return w

    def embed(self, values, scale, level, ntt, mont, scale_up, signed, to_p=False) -> np.ndarray:
        """EmbedScale (:268-334) into a ring.Poly, or the P half of a ringqp.Poly with to_p: [level + 1][N]"""
        return self._finish(self.ring_t2q(self.encode_ring_t(values, scale, signed), level, scale_up, to_p), to_p, level, ntt, mont)

    def encode_coeffs(self, values, scale, level, ntt, signed) -> np.ndarray:
        """Encode with IsBatched = false (:147-198), N_T = N"""
        assert self.gap == 1
        pt = np.zeros((1, self.N), dtype=np.uint64)
        w = reduce_words(values, self.T, signed)
        pt[0, : len(w)] = w
        return self._finish(self.ring_t2q(self.mul_scalar_t(pt, scale), level, True), False, level, ntt, False)

    def decode(self, pt, scale, level, batched, ntt, signed) -> np.ndarray:
        """Decode (:470-526): [N_T]"""
        w = np.asarray(pt, dtype=np.uint64)[: level + 1]
        if ntt:
            w = self.oQ.INTT(w, level=level)
        pT = self.ring_q2t(w, level, True)
        if batched:
            return self.decode_ring_t(pT, scale, signed)
        assert self.gap == 1
        return self.centre(self.mul_scalar_t(pT, pow(int(scale), self.T - 2, self.T))[0], signed)


@functools.lru_cache(maxsize=None)
def _crt_constants(mods: tuple):
    Q = prod(mods)
    return Q, [(Q // m) * pow(Q // m, -1, m) for m in mods]


def crt(words, mods) -> int:
    Q, c = _crt_constants(tuple(int(m) for m in mods))
    return sum(int(w) * k for w, k in zip(words, c)) % Q


def centred_value(words, mods) -> int:
    """PolyToBigintCentered (ring/ring.go:469-509) of one coefficient: x >= Q >> 1 -> x - Q"""
    Q = prod(mods)
    x = crt(words, mods)
    return x - Q if x >= (Q >> 1) else x


def words_of(x: int, mods) -> list:
    return [x % m for m in mods]
