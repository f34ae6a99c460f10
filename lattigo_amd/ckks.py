"""ckks.Encoder (schemes/ckks/encoder.go), the double-precision path the reference takes when prec <= 53, on the device
(include/hering_ckks_encoder.h): Encode / EncodeQP / Embed, Decode / DecodePublic and the special FFT / IFFT, numpy arrays in
and out.  A plaintext is a Poly plus the metadata the reference keeps in rlwe.MetaData, passed as keyword arguments."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import H, check, load
from .ring import Poly, Ring

_f64p = C.POINTER(C.c_double)


def _dp(a):
    return a.ctypes.data_as(_f64p)


def roots_host(nth_root: int) -> np.ndarray:
    """GetRootsComplex128(nth_root) (schemes/ckks/utils.go:53-77) as complex128 [nth_root + 1]; no device needed."""
    out = np.zeros(2 * (nth_root + 1), dtype=np.float64)
    check(load().he_ckks_roots_host(nth_root, _dp(out)))
    return out.view(np.complex128)


class Encoder:
    """ckks.NewEncoder(parameters) with prec <= 53.  `ringQ`: Parameters.RingQ(); `ringP`: Parameters.RingP() or None (needed by
    EncodeQP only); `roots`: None for the built-in table, or complex128 [NthRoot + 1] (a Go host passes GetRootsComplex128's
    words and gets Go's bits)."""

    def __init__(self, ringQ: Ring, ringP: Ring | None = None, roots=None):
        self.ringQ, self.ringP = ringQ, ringP
        h = H()
        r = None
        if roots is not None:
            r = np.ascontiguousarray(roots, dtype=np.complex128).view(np.float64)
            if r.size != 2 * (ringQ.NthRoot() + 1):
                raise ValueError(f"the table of roots holds {r.size // 2} values, NthRoot + 1 = {ringQ.NthRoot() + 1} expected")
        check(load().he_ckks_encoder_create(ringQ.h, ringP.h if ringP is not None else 0, _dp(r) if r is not None else None, C.byref(h)))
        self.h = h.value
        info = (C.c_int * 4)()
        check(load().he_ckks_encoder_info(self.h, info))
        self.logM, self.LogMaxSlots, self.FFTOneWorkgroupMaxLogN, self.DecodeMaxLimbs = (int(x) for x in info)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                load().he_ckks_encoder_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def Roots(self) -> np.ndarray:
        """the table the encoder holds, complex128 [NthRoot + 1]"""
        out = np.zeros(2 * ((1 << self.logM) + 1), dtype=np.float64)
        check(load().he_ckks_encoder_roots(self.h, _dp(out)))
        return out.view(np.complex128)

    # -- Encoder.FFT / Encoder.IFFT (:765-820): values complex [n] or [batch][n], n = 2^logN; returns a new array
    def _fft(self, values, logN, inverse):
        v = np.array(values, dtype=np.complex128, order="C")
        n = 1 << logN
        if v.ndim not in (1, 2) or v.shape[-1] != n:
            raise ValueError(f"values of shape {v.shape}, [batch][{n}] expected")
        batch = 1 if v.ndim == 1 else v.shape[0]
        check((load().he_ckks_ifft if inverse else load().he_ckks_fft)(self.h, logN, batch, _dp(v.view(np.float64))))
        return v

    def FFT(self, values, logN: int) -> np.ndarray:
        return self._fft(values, logN, False)

    def IFFT(self, values, logN: int) -> np.ndarray:
        return self._fft(values, logN, True)

    @staticmethod
    def _values(values):
        v = np.asarray(values)
        cplx = np.iscomplexobj(v)
        v = np.ascontiguousarray(v, dtype=np.complex128 if cplx else np.float64)
        if v.ndim == 1:
            v = v[None, :]
        if v.ndim != 2:
            raise ValueError("values: [n] or [batch][n]")
        return v, cplx

    def Encode(self, values, pt: Poly, *, Scale: float, LogSlots: int | None = None, IsBatched: bool = True, IsNTT: bool = True,
               IsMontgomery: bool = False, level: int | None = None):
        """Encoder.Encode (:156): values [n] or [batch][n] (float64 or complex128) into pt (batch entries) at `level` (default:
        pt.Level())."""
        v, cplx = self._values(values)
        level = pt.Level() if level is None else level
        ls = self.LogMaxSlots if LogSlots is None else LogSlots
        check(load().he_ckks_encode(self.h, level, ls, float(Scale), int(IsBatched), int(IsNTT), int(IsMontgomery), _dp(v.view(np.float64)),
                                    v.shape[1], int(cplx), v.shape[0], pt.h))
        return pt

    def Embed(self, values, polyOut: Poly, *, Scale: float, LogSlots: int | None = None, IsNTT: bool = True, IsMontgomery: bool = False,
              level: int | None = None):
        """Encoder.Embed (:208) into a ring.Poly: the batched arm of Encode."""
        return self.Encode(values, polyOut, Scale=Scale, LogSlots=LogSlots, IsBatched=True, IsNTT=IsNTT, IsMontgomery=IsMontgomery, level=level)

    def EncodeQP(self, values, polyQ: Poly, polyP: Poly | None, *, Scale: float, LogSlots: int | None = None, IsNTT: bool = True,
                 IsMontgomery: bool = True, levelQ: int | None = None, levelP: int | None = None):
        """Embed into a ringqp.Poly (:321-328): one IFFT feeding polyQ and polyP (None: P.Level() = -1)."""
        v, cplx = self._values(values)
        levelQ = polyQ.Level() if levelQ is None else levelQ
        levelP = (-1 if polyP is None else polyP.Level()) if levelP is None else levelP
        ls = self.LogMaxSlots if LogSlots is None else LogSlots
        check(load().he_ckks_encode_qp(self.h, levelQ, levelP, ls, float(Scale), int(IsNTT), int(IsMontgomery), _dp(v.view(np.float64)), v.shape[1],
                                       int(cplx), v.shape[0], polyQ.h, polyP.h if polyP is not None else 0))
        return polyQ, polyP

    def DecodePublic(self, pt: Poly, *, Scale: float, logprec: float = 0.0, LogSlots: int | None = None, IsBatched: bool = True,
                     IsNTT: bool = True, level: int | None = None, complex_out: bool = True) -> np.ndarray:
        """Encoder.DecodePublic (:199): [batch][slots] (batched) or [batch][N]; complex128, or float64 with complex_out = False."""
        level = pt.Level() if level is None else level
        ls = self.LogMaxSlots if LogSlots is None else LogSlots
        n = (1 << ls) if IsBatched else pt.N
        out = np.zeros((pt.batch, n), dtype=np.complex128 if complex_out else np.float64)
        check(load().he_ckks_decode(self.h, level, ls, float(Scale), int(IsBatched), int(IsNTT), float(logprec), pt.h, int(complex_out),
                                    _dp(out.view(np.float64))))
        return out

    def Decode(self, pt: Poly, **kw) -> np.ndarray:
        """Encoder.Decode (:192): DecodePublic with logprec = 0."""
        return self.DecodePublic(pt, logprec=0.0, **kw)
