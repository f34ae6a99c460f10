"""bgv.Encoder (schemes/bgv/encoder.go), the encoder of BGV and BFV, on the device (include/hering_bgv_encoder.h): Encode / Embed /
EncodeQP, Decode, EncodeRingT / DecodeRingT, RingT2Q / RingQ2T, numpy arrays in and out.  The dtype of the values decides the
path: int64 is the reference's []int64, anything else is taken as uint64.  A plaintext is a Poly plus the metadata the reference
keeps in rlwe.MetaData, passed as keyword arguments."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import H, check, load, u64p
from .ring import Poly, Ring


def _up(a):
    return a.ctypes.data_as(u64p)


class Encoder:
    """bgv.NewEncoder(parameters).  `ringQ`: Parameters.RingQ(); `ringT`: Parameters.RingT(), one modulus T and degree
    min(N, 2^(v2(T - 1) - 1)); `ringP`: Parameters.RingP() or None (needed by EncodeQP and RingT2Q(to_p=True) only)."""

    def __init__(self, ringQ: Ring, ringT: Ring, ringP: Ring | None = None):
        self.ringQ, self.ringT, self.ringP = ringQ, ringT, ringP
        h = H()
        check(load().he_bgv_encoder_create(ringQ.h, ringP.h if ringP is not None else 0, ringT.h, C.byref(h)))
        self.h = h.value
        info = (C.c_int * 4)()
        check(load().he_bgv_encoder_info(self.h, info))
        self.LogMaxSlots, self.LogGap, self.RingQ2TMaxLimbs = int(info[0]), int(info[1]), int(info[2])
        self.MaxSlots = 1 << self.LogMaxSlots

    def __del__(self):
        try:
            if getattr(self, "h", None):
                load().he_bgv_encoder_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def IndexMatrix(self) -> np.ndarray:
        """permuteMatrix(LogMaxSlots) (:110-133) as the encoder holds it, uint64 [MaxSlots]"""
        out = np.zeros(self.MaxSlots, dtype=np.uint64)
        check(load().he_bgv_encoder_index(self.h, _up(out)))
        return out

    @staticmethod
    def _values(values):
        """([batch][n] words as uint64, is_signed)"""
        v = np.asarray(values)
        signed = v.dtype == np.int64
        v = np.ascontiguousarray(v, dtype=np.int64 if signed else np.uint64)
        if v.ndim == 1:
            v = v[None, :]
        if v.ndim != 2:
            raise ValueError("values: [n] or [batch][n]")
        return v.view(np.uint64), signed

    def _out(self, batch, n, signed):
        return np.zeros((batch, n), dtype=np.uint64), (lambda o: o.view(np.int64) if signed else o)

    def EncodeRingT(self, values, scale: int, pT: Poly):
        """EncodeRingT (:203): values [n] or [batch][n] into pT (ringT, batch entries)"""
        v, signed = self._values(values)
        check(load().he_bgv_encode_ring_t(self.h, int(scale), _up(v), v.shape[1], int(signed), v.shape[0], pT.h))
        return pT

    def DecodeRingT(self, pT: Poly, scale: int, signed: bool = False) -> np.ndarray:
        """DecodeRingT (:341): [batch][MaxSlots], int64 (centred) with signed, else uint64"""
        out, fin = self._out(pT.batch, self.MaxSlots, signed)
        check(load().he_bgv_decode_ring_t(self.h, int(scale), pT.h, int(signed), _up(out)))
        return fin(out)

    def RingT2Q(self, level: int, scaleUp: bool, pT: Poly, pQ: Poly, to_p: bool = False):
        """RingT2Q (:378); to_p: pQ is a polynomial of ringP"""
        check(load().he_bgv_ring_t2q(self.h, level, int(scaleUp), int(to_p), pT.h, pQ.h))
        return pQ

    def RingQ2T(self, level: int, scaleDown: bool, pQ: Poly, pT: Poly):
        """RingQ2T (:412)"""
        check(load().he_bgv_ring_q2t(self.h, level, int(scaleDown), pQ.h, pT.h))
        return pT

    def Encode(self, values, pt: Poly, *, Scale: int = 1, IsBatched: bool = True, IsNTT: bool = True, IsMontgomery: bool = False,
               level: int | None = None, scaleUp: bool = True):
        """Encoder.Encode (:143): values [n] or [batch][n] into pt (batch entries) at `level` (default: pt.Level())"""
        v, signed = self._values(values)
        level = pt.Level() if level is None else level
        check(load().he_bgv_encode(self.h, level, int(Scale), int(IsBatched), int(IsNTT), int(IsMontgomery), int(scaleUp), _up(v), v.shape[1],
                                   int(signed), v.shape[0], pt.h))
        return pt

    def Embed(self, values, polyOut: Poly, *, Scale: int = 1, IsNTT: bool = True, IsMontgomery: bool = False, level: int | None = None):
        """Encoder.Embed (:336) into a ring.Poly: EmbedScale without the factor T^-1"""
        return self.Encode(values, polyOut, Scale=Scale, IsBatched=True, IsNTT=IsNTT, IsMontgomery=IsMontgomery, level=level, scaleUp=False)

    def EncodeQP(self, values, polyQ: Poly, polyP: Poly | None, *, Scale: int = 1, IsNTT: bool = True, IsMontgomery: bool = True,
                 levelQ: int | None = None, levelP: int | None = None, scaleUp: bool = False):
        """EmbedScale into a ringqp.Poly (:280-311): one transform modulo T feeding polyQ and polyP (None: P.Level() = -1)"""
        v, signed = self._values(values)
        levelQ = polyQ.Level() if levelQ is None else levelQ
        levelP = (-1 if polyP is None else polyP.Level()) if levelP is None else levelP
        check(load().he_bgv_encode_qp(self.h, levelQ, levelP, int(Scale), int(IsNTT), int(IsMontgomery), int(scaleUp), _up(v), v.shape[1], int(signed),
                                      v.shape[0], polyQ.h, polyP.h if polyP is not None else 0))
        return polyQ, polyP

    def Decode(self, pt: Poly, *, Scale: int = 1, IsBatched: bool = True, IsNTT: bool = True, level: int | None = None,
               signed: bool = False) -> np.ndarray:
        """Encoder.Decode (:470): [batch][MaxSlots], int64 (centred) with signed, else uint64"""
        level = pt.Level() if level is None else level
        out, fin = self._out(pt.batch, self.MaxSlots, signed)
        check(load().he_bgv_decode(self.h, level, int(Scale), int(IsBatched), int(IsNTT), pt.h, int(signed), _up(out)))
        return fin(out)
