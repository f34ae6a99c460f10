"""sampling.PRNG and the ring samplers on the device (include/hering_sampler.h): ring.UniformSampler / ringqp.UniformSampler
(ring/sampler_uniform.go, ring/ringqp/samplers.go), ring.GaussianSampler (ring/sampler_gaussian.go) and ring.TernarySampler with a
density (ring/sampler_ternary.go).  Each sampler is an exact function of the byte stream its PRNG serves: the words, the bytes
consumed and the position of the source afterwards are the reference's.  A Poly of B entries is B successive Reads."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import H, HeringError, PRNG_READ_FN, check, load
from .ring import Poly, Ring


class PRNG:
    """sampling.PRNG.  PRNG(): crypto/rand's analogue, getrandom(2).  PRNG(read): `read(n)` returns the next n bytes of any
    io.Reader (a bytes-like object; fewer than n bytes, or an exception, is a failed read).  The library may fetch ahead; Position()
    counts the bytes consumed in the reference's sense.  An exception the reader raised is the __cause__ of the HeringError
    (HE_EPRNG) that the sampler or encryptor call raises."""

    def __init__(self, read=None):
        h = H()
        self._read, self._cb, self.error = read, None, None
        if read is None:
            check(load().he_prng_create_system(C.byref(h)))
        else:
            def cb(_user, dst, n):
                try:
                    data = bytes(self._read(n))
                    if len(data) != n:
                        return 1
                    C.memmove(dst, data, n)
                    return 0
                except Exception as e:  # a callback must not raise through the C frames
                    self.error = e
                    return 2
            self._cb = PRNG_READ_FN(cb)
            check(load().he_prng_create_callback(self._cb, None, C.byref(h)))
        self.h = h.value

    def __del__(self):
        try:
            if getattr(self, "h", None):
                load().he_prng_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def check(self, rc: int):
        """check(rc) for a call that reads this source: a failure carries the reader's exception, when it raised one"""
        try:
            check(rc)
        except HeringError as e:
            cause, self.error = self.error, None
            if cause is not None:
                raise e from cause
            raise

    def Position(self) -> int:
        out = (C.c_uint64 * 2)()
        check(load().he_prng_position(self.h, out))
        return int(out[0])

    def FetchedAhead(self) -> int:
        out = (C.c_uint64 * 2)()
        check(load().he_prng_position(self.h, out))
        return int(out[1])


class UniformSampler:
    """ring.NewUniformSampler(prng, baseRing); with ringP, ringqp.NewUniformSampler(prng, ringqp.Ring{ringQ, ringP}), whose
    polynomials are (Q, P) pairs."""

    def __init__(self, prng: PRNG, baseRing: Ring, ringP: Ring | None = None):
        self.prng, self.baseRing, self.ringP = prng, baseRing, ringP

    def AtLevel(self, level: int, levelP: int | None = None) -> "UniformSampler":
        return UniformSampler(self.prng, self.baseRing.AtLevel(level), None if self.ringP is None else self.ringP.AtLevel(levelP))

    def _read(self, pol, add):
        q, p = (pol, None) if self.ringP is None else pol
        self.prng.check(load().he_sampler_uniform_read(self.baseRing.h, self.baseRing.Level(), self.ringP.h if p is not None else 0,
                                             self.ringP.Level() if p is not None else 0, self.prng.h, add, q.h, p.h if p is not None else 0))

    def Read(self, pol):
        self._read(pol, 0)

    def ReadAndAdd(self, pol):
        self._read(pol, 1)

    def ReadNew(self, batch: int = 1):
        pol = self.baseRing.NewPoly(batch) if self.ringP is None else (self.baseRing.NewPoly(batch), self.ringP.NewPoly(batch))
        self.Read(pol)
        return pol


class GaussianSampler:
    """ring.NewGaussianSampler(prng, baseRing, DiscreteGaussian{Sigma, Bound}, montgomery)"""

    def __init__(self, prng: PRNG, baseRing: Ring, Sigma: float, Bound: float, montgomery: bool):
        self.prng, self.baseRing, self.Sigma, self.Bound, self.montgomery = prng, baseRing, float(Sigma), float(Bound), bool(montgomery)

    def AtLevel(self, level: int) -> "GaussianSampler":
        return GaussianSampler(self.prng, self.baseRing.AtLevel(level), self.Sigma, self.Bound, self.montgomery)

    def _read(self, pol: Poly, add):
        self.prng.check(load().he_sampler_gaussian_read(self.baseRing.h, self.baseRing.Level(), self.prng.h, self.Sigma, self.Bound, int(self.montgomery),
                                              add, pol.h))

    def Read(self, pol: Poly):
        self._read(pol, 0)

    def ReadAndAdd(self, pol: Poly):
        self._read(pol, 1)

    def ReadNew(self, batch: int = 1) -> Poly:
        pol = self.baseRing.NewPoly(batch)
        self.Read(pol)
        return pol


class TernarySampler:
    """ring.NewTernarySampler(prng, baseRing, Ternary{P: P}, montgomery).  The sparse form (Ternary{H: h}) is keygen.SparseTernarySampler."""

    def __init__(self, prng: PRNG, baseRing: Ring, P: float, montgomery: bool, _words=None):
        """_words: (x0, x1), the matrix words of he_debug_sampler_ternary_words instead of those of P (tests)"""
        self.prng, self.baseRing, self.P, self.montgomery, self.words = prng, baseRing, float(P), bool(montgomery), _words

    def AtLevel(self, level: int) -> "TernarySampler":
        return TernarySampler(self.prng, self.baseRing.AtLevel(level), self.P, self.montgomery, self.words)

    def _read(self, pol: Poly, add):
        if self.words is not None:
            self.prng.check(load().he_debug_sampler_ternary_words(self.baseRing.h, self.baseRing.Level(), self.prng.h, self.words[0], self.words[1],
                                                        int(self.montgomery), add, pol.h))
            return
        self.prng.check(load().he_sampler_ternary_read(self.baseRing.h, self.baseRing.Level(), self.prng.h, self.P, int(self.montgomery), add, pol.h))

    def Read(self, pol: Poly):
        self._read(pol, 0)

    def ReadAndAdd(self, pol: Poly):
        self._read(pol, 1)

    def ReadNew(self, batch: int = 1) -> Poly:
        pol = self.baseRing.NewPoly(batch)
        self.Read(pol)
        return pol


def GaussianTables():
    """(kn uint32[128], wn float32[128], fn float32[128]) as the library generates them (he_gaussian_tables_host)"""
    out = np.zeros(384, dtype=np.uint32)
    check(load().he_gaussian_tables_host(out.ctypes.data_as(C.POINTER(C.c_uint32))))
    return out[:128].copy(), out[128:256].view(np.float32).copy(), out[256:].view(np.float32).copy()


def TernaryMatrix(P: float):
    """matrixProba of computeMatrixTernary(1 - P) as uint8 [2][55] (he_ternary_matrix_host)"""
    out = (C.c_uint64 * 2)()
    check(load().he_ternary_matrix_host(float(P), out))
    return np.array([[(int(out[r]) >> (55 - j)) & 1 for j in range(55)] for r in range(2)], dtype=np.uint8)
