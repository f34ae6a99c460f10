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


# ---- include/hering_ckks_evaluator.h: the evaluator's entries over component lists ------------------------------------------------
def _handles(polys):
    return (H * len(polys))(*[p.h for p in polys])


def _res(words, level):
    """residues on the limbs 0 .. level as (array kept alive, pointer), or (None, None)"""
    if words is None:
        return None, None
    w = np.ascontiguousarray(words, dtype=np.uint64)
    if w.size < level + 1:
        raise ValueError("one residue per limb is needed")
    return w, w.ctypes.data_as(C.POINTER(C.c_uint64))


def ct_add(ring: Ring, op0, op1, out, *, sub: bool = False, scaled: int = 0, ratio=None):
    """he_ckks_add at ring.level: evaluateInPlace (schemes/ckks/evaluator.go:221-408) with Ring.Add / Ring.Sub over the component
    lists op0, op1 -> out (len(out) = max), one launch; scaled = 1 / 2: that operand is first multiplied by the integer with the
    residues `ratio`."""
    _keep, r = _res(ratio, ring.level)
    check(load().he_ckks_add(ring.h, ring.level, int(sub), len(op0), _handles(op0), len(op1), _handles(op1), scaled, r, len(out), _handles(out)))


def ct_scalar(ring: Ring, op: int, op0, s0, s1, out, *, pre=None):
    """he_ckks_scalar at ring.level: evaluateWithScalar (:410-424); op 0 add, 1 sub, 2 mul, 3 mul-then-add onto out (pre: the
    residues of the integer out is multiplied by first)."""
    _k0, a = _res(s0, ring.level)
    _k1, b = _res(s1, ring.level)
    _k2, p = _res(pre, ring.level)
    check(load().he_ckks_scalar(ring.h, ring.level, op, len(op0), _handles(op0), a, b, p, _handles(out)))


def ct_mul_pt(ring: Ring, ct, pt: Poly, out, *, then_add: bool = False, pre=None):
    """he_ckks_mul_pt at ring.level: the plaintext branches of mulRelin (:842-869) and mulRelinThenAdd (:1158-1170)."""
    _keep, p = _res(pre, ring.level)
    check(load().he_ckks_mul_pt(ring.h, ring.level, len(ct), _handles(ct), pt.h, int(then_add), p, _handles(out)))


def ct_mul_relin_then_add(evaluator, level: int, a, b, rlk, out, *, pre=None):
    """he_ckks_mul_relin_then_add: the ciphertext x ciphertext branch of mulRelinThenAdd (:1104-1155); rlk None: out has three
    components, else two."""
    _keep, p = _res(pre, level)
    check(load().he_ckks_mul_relin_then_add(evaluator.h, level, a[0].h, a[1].h, b[0].h, b[1].h, rlk.h if rlk is not None else 0, p,
                                            out[0].h, out[1].h, out[2].h if len(out) > 2 else 0))


# ---- ckks.Parameters (light) and ckks.Evaluator (schemes/ckks/evaluator.go) ---------------------------------------------------------
class Parameters:
    """What ckks.Evaluator reads of ckks.Parameters: the ring, the default scale and EncodingPrecision (schemes/ckks/params.go:
    185-195).  LevelsConsumedPerRescaling is 1: a default scale above 2^60 (the 128-bit-precision parameter sets, which need the
    big-float encoder) is refused."""

    def __init__(self, ringQ: Ring, DefaultScale, ringP: Ring | None = None):
        from .polyeval import CKKSScheme
        from .rlwe import Scale
        self.ringQ, self.ringP, self.DefaultScale = ringQ, ringP, Scale(DefaultScale)
        if self.DefaultScale.Cmp(1 << 60) > 0:
            raise ValueError("LevelsConsumedPerRescaling = 2 (a default scale above 2^60) needs the arbitrary-precision encoder, which is not provided")
        self.scheme = CKKSScheme.for_ring(ringQ, self.DefaultScale.Float64())

    def RingQ(self) -> Ring:
        return self.ringQ

    def MaxLevel(self) -> int:
        return self.ringQ.MaxLevel()

    def EncodingPrecision(self) -> int:
        return self.scheme.EncodingPrecision

    def LevelsConsumedPerRescaling(self) -> int:
        return 1

    def NTTFlag(self) -> bool:
        return True

    def Q(self):
        return [int(q) for q in self.ringQ.ModuliChain()]


def NewCiphertext(params: Parameters, degree: int, level: int, batch: int = 1):
    from .rlwe import Ciphertext, MetaData
    return Ciphertext(params.ringQ, degree, level, batch,
                      MetaData_=MetaData(params.DefaultScale, LogDimensions=(0, params.ringQ.N.bit_length() - 2)))  # LogMaxDimensions


_OPERAND_ERROR = ("op1.(type) must be rlwe.ElementInterface[ring.Poly], complex128, float64, int, int64, uint, uint64, *big.Int, *big.Float, "
                  "*bignum.Complex, []complex128, []float64, []*big.Float or []*bignum.Complex, but is %s")


def _is_scalar(x) -> bool:
    """complex128, float64, int, int64, uint, uint64 (numpy's scalar types included), *big.Int; a Fraction stands for *big.Float"""
    from fractions import Fraction
    return not isinstance(x, (bool, np.bool_)) and isinstance(x, (int, float, complex, Fraction, np.integer, np.floating, np.complexfloating))


def _scalar(x):
    from fractions import Fraction
    if isinstance(x, (Fraction, int)) and not isinstance(x, np.integer):
        return x
    if isinstance(x, np.integer):
        return int(x)
    return complex(x) if isinstance(x, (complex, np.complexfloating)) else float(x)


def _is_vector(x) -> bool:
    return isinstance(x, (np.ndarray, list, tuple))


def _is_element(x) -> bool:
    return hasattr(x, "Value") and hasattr(x, "MetaData")


class Evaluator:
    """ckks.Evaluator over device ciphertexts (lattigo_amd.rlwe.Ciphertext / Plaintext): the reference's method names, argument
    order (outputs last) and error texts.  `evaluator`: the rlwe.Evaluator of the parameters (lattigo_amd.rlwe.Evaluator); `rlk`:
    the relinearization key or None.  Operands (rlwe.Operand): a Ciphertext or Plaintext, or a scalar (int, float, complex,
    Fraction).  Metadata handling restates InitOutputBinaryOp / InitOutputUnaryOp (core/rlwe/evaluator.go:119-196), the scale
    matching evaluateInPlace (:221-408) and the scalar words bigComplexToRNSScalar (scaling.go:10-43, shared with
    lattigo_amd.polyeval)."""

    def __init__(self, params: Parameters, evaluator, rlk=None, gks=None, encoder: "Encoder | None" = None):
        """rlk: the relinearization key; gks: the rlwe.GaloisKeySet of the rotations; encoder: the ckks.Encoder vector operands are
        encoded with (made on first use when None).  Together rlk and gks are the reference's rlwe.EvaluationKeySet."""
        self.params, self.ev, self.rlk, self.gks, self.Encoder = params, evaluator, rlk, gks, encoder
        self._rot = None

    def WithKey(self, rlk, gks=None) -> "Evaluator":
        return Evaluator(self.params, self.ev, rlk, gks, self.Encoder)

    def _rotations(self, name):
        from .rlwe import CKKSRotations
        if self.gks is None:
            raise ValueError(f"cannot {name}: EvaluationKeySet is nil")
        if self._rot is None:
            self._rot = CKKSRotations(self.ev, self.gks)
        return self._rot

    def _encode(self, values, level, meta, scale, batch):
        """a vector operand: Encoder.Encode(op1, pt) into a scratch plaintext with `meta` at `scale` (:98-104, :681-694, :1012-1021)"""
        from .rlwe import Plaintext
        if self.Encoder is None:
            self.Encoder = Encoder(self.params.ringQ, self.params.ringP)
        v = np.asarray(values)
        if v.ndim != 1 or not (np.issubdtype(v.dtype, np.floating) or np.issubdtype(v.dtype, np.complexfloating) or np.issubdtype(v.dtype, np.integer)):
            raise ValueError(_OPERAND_ERROR % type(values).__name__)
        pt = Plaintext(self.params.ringQ, level, 1, MetaData_=meta.copy())
        pt.Scale = scale
        self.Encoder.Encode(v.astype(np.complex128 if np.iscomplexobj(v) else np.float64), pt.Value[0], Scale=pt.Scale.Float64(),
                            LogSlots=meta.LogDimensions[1], IsBatched=meta.IsBatched, level=level)
        return pt

    def GetParameters(self) -> Parameters:
        return self.params

    # -- core/rlwe/evaluator.go:119-196
    def InitOutputBinaryOp(self, op0, op1, opInTotalMaxDegree, opOut):
        degree = max(op0.Degree(), op1.Degree(), opOut.Degree())
        level = min(op0.Level(), op1.Level(), opOut.Level())
        tot = op0.Degree() + op1.Degree()
        if tot == 0:
            raise ValueError("op0 and op1 cannot be both plaintexts")
        if tot > opInTotalMaxDegree:
            raise ValueError(f"op0 and op1 total degree cannot exceed {opInTotalMaxDegree} but is {tot}")
        if op0.IsNTT != op1.IsNTT or op0.IsNTT != self.params.NTTFlag():
            raise ValueError("op0.El().IsNTT or op1.El().IsNTT != true")
        opOut.IsNTT = op0.IsNTT
        if op0.IsBatched != op1.IsBatched:
            raise ValueError("op1.El().IsBatched != opOut.El().IsBatched")
        opOut.IsBatched = op0.IsBatched
        opOut.LogDimensions = (max(op0.LogDimensions[0], op1.LogDimensions[0]), max(op0.LogDimensions[1], op1.LogDimensions[1]))
        return degree, level

    def InitOutputUnaryOp(self, op0, opOut):
        if op0.IsNTT != self.params.NTTFlag():
            raise ValueError("op0.IsNTT() != true")
        opOut.IsNTT, opOut.IsBatched, opOut.LogDimensions = op0.IsNTT, op0.IsBatched, op0.LogDimensions
        return max(op0.Degree(), opOut.Degree()), min(op0.Level(), opOut.Level())

    def _ring(self, level) -> Ring:
        return self.params.ringQ.AtLevel(level)

    def _scalar_words(self, level, scale, c):
        from fractions import Fraction
        from .rlwe import Scale
        v = scale.Value if isinstance(scale, Scale) else Fraction(scale)
        s0, s1 = self.params.scheme._rns(level, v, c)
        return np.array(s0, dtype=np.uint64), np.array(s1, dtype=np.uint64)

    def _int_words(self, level, n: int):
        """the words of Evaluator.Mul(ct, n, .) for an integer n: the scalar path with scale 1 (:645-646)"""
        return self._scalar_words(level, 1, n)[0]

    # -- Add / Sub (:51-219)
    def _add_sub(self, op0, op1, opOut, sub: bool, name: str):
        if _is_scalar(op1) or _is_vector(op1):
            try:
                _, level = self.InitOutputUnaryOp(op0, opOut)
            except ValueError as e:
                raise ValueError(f"cannot {name}: {e}") from None
            opOut.Resize(op0.Degree(), level)
            if _is_vector(op1):  # :88-109: the plaintext takes op0's metadata, "notably matches scales"
                pt = self._encode(op1, level, op0.MetaData, op0.Scale, op0.batch)
                self._evaluate_in_place(level, op0, pt, opOut, sub)
                return
            s0, s1 = self._scalar_words(level, op0.Scale, _scalar(op1))
            ct_scalar(self._ring(level), 1 if sub else 0, op0.Value[: opOut.Degree() + 1], s0, s1, opOut.Value)
            return
        if not _is_element(op1):
            raise ValueError("invalid op1.(type): must be rlwe.ElementInterface[ring.Poly], complex128, float64, int, int64, uint, uint64, "
                             "*big.Int, *big.Float, *bignum.Complex, []complex128, []float64, []*big.Float or []*bignum.Complex, but is "
                             + type(op1).__name__)
        try:
            degree, level = self.InitOutputBinaryOp(op0, op1, op0.Degree() + op1.Degree(), opOut)
        except ValueError as e:
            raise ValueError(f"cannot {name}: {e}") from None
        opOut.Resize(degree, level)
        self._evaluate_in_place(level, op0, op1, opOut, sub)

    def _evaluate_in_place(self, level, c0, c1, opOut, sub):
        """evaluateInPlace (:221-408) and the Neg of Sub (:152-156): whichever of its nine branches is taken -- opOut is c0, is c1 or
        neither, times the comparison of the scales -- the operand of the smaller scale is multiplied by the truncated ratio and
        the words of opOut are those of one he_ckks_add call; opOut.Scale is the larger scale"""
        cmp = c0.Scale.Cmp(c1.Scale)
        scaled, ratio = 0, None
        if cmp != 0:
            big, small = (c0.Scale, c1.Scale) if cmp == 1 else (c1.Scale, c0.Scale)
            ratio_int = big.Div(small).Int()
            if ratio_int > 0:
                scaled, ratio = (2 if cmp == 1 else 1), self._int_words(level, ratio_int)
        n_out = max(c0.Degree(), c1.Degree()) + 1
        ct_add(self._ring(level), c0.Value, c1.Value, opOut.Value[:n_out], sub=sub, scaled=scaled, ratio=ratio)
        opOut.Scale = c0.Scale.Max(c1.Scale)

    def Add(self, op0, op1, opOut):
        self._add_sub(op0, op1, opOut, False, "Add")

    def Sub(self, op0, op1, opOut):
        self._add_sub(op0, op1, opOut, True, "Sub")

    def AddNew(self, op0, op1):
        opOut = NewCiphertext(self.params, op0.Degree(), op0.Level(), op0.batch)
        self.Add(op0, op1, opOut)
        return opOut

    def SubNew(self, op0, op1):
        opOut = NewCiphertext(self.params, op0.Degree(), op0.Level(), op0.batch)
        self.Sub(op0, op1, opOut)
        return opOut

    # -- Mul / MulRelin (:596-872)
    def _mul(self, op0, op1, opOut, relin: bool, name: str):
        from .rlwe import Scale
        if _is_scalar(op1) or _is_vector(op1):
            # (MulRelin with a scalar or a vector is Mul, :756-759)
            try:
                _, level = self.InitOutputUnaryOp(op0, opOut)
            except ValueError as e:
                raise ValueError(f"cannot {name}: {e}") from None
            opOut.Resize(op0.Degree(), level)
            if _is_vector(op1):  # :668-701: encoded at scale q_level, then the plaintext branch of mulRelin
                pt = self._encode(op1, level, op0.MetaData, Scale(self.params.Q()[level]), op0.batch)
                opOut.Scale = op0.Scale.Mul(pt.Scale)
                ct_mul_pt(self._ring(level), op0.Value, pt.Value[0], opOut.Value)
                return
            op1 = _scalar(op1)
            scale = Scale(1) if self.params.scheme._is_int(op1) else Scale(self.params.Q()[level])  # :644-655
            s0, s1 = self._scalar_words(level, scale, op1)
            ct_scalar(self._ring(level), 2, op0.Value[: opOut.Degree() + 1], s0, s1, opOut.Value)
            opOut.Scale = op0.Scale.Mul(scale)
            return
        if not _is_element(op1):
            raise ValueError(_OPERAND_ERROR % type(op1).__name__)
        try:
            _, level = self.InitOutputBinaryOp(op0, op1, 2, opOut)
        except ValueError as e:
            raise ValueError(f"cannot {name}: {e}") from None
        opOut.Scale = op0.Scale.Mul(op1.Scale)  # :774
        if op0.Degree() == 1 and op1.Degree() == 1:
            if relin and self.rlk is None:  # (:824-828, wrapped by :756 and :749)
                raise ValueError(f"cannot {name}: cannot {name}: Relinearize: EvaluationKeySet is nil")
            opOut.Resize(1 if relin else 2, level)
            self.ev.CKKSMulRelin(level, op0.Value, op1.Value, self.rlk if relin else None, opOut.Value)
        else:
            ct, pt = (op1, op0) if op0.Degree() == 0 else (op0, op1)
            opOut.Resize(max(op0.Degree(), op1.Degree()), level)
            ct_mul_pt(self._ring(level), ct.Value, pt.Value[0], opOut.Value)

    def Mul(self, op0, op1, opOut):
        self._mul(op0, op1, opOut, False, "Mul")

    def MulRelin(self, op0, op1, opOut):
        self._mul(op0, op1, opOut, True, "MulRelin")

    def MulNew(self, op0, op1):
        deg = op0.Degree() + op1.Degree() if _is_element(op1) else op0.Degree()
        lvl = min(op0.Level(), op1.Level()) if _is_element(op1) else op0.Level()
        opOut = NewCiphertext(self.params, deg, lvl, op0.batch)
        self.Mul(op0, op1, opOut)
        return opOut

    def MulRelinNew(self, op0, op1):
        opOut = NewCiphertext(self.params, 1, min(op0.Level(), op1.Level()), op0.batch)
        self.MulRelin(op0, op1, opOut)
        return opOut

    # -- MulThenAdd / MulRelinThenAdd (:909-1173)
    def _mul_then_add(self, op0, op1, opOut, relin: bool, name: str):
        from .rlwe import Scale
        if _is_scalar(op1) or _is_vector(op1):
            # (MulRelinThenAdd with a scalar or a vector is MulThenAdd, :1075-1076)
            try:
                _, level = self.InitOutputUnaryOp(op0, opOut)
            except ValueError as e:
                raise ValueError(f"cannot MulThenAdd: {e}") from None
            opOut.Resize(op0.Degree(), opOut.Level())
            vector = _is_vector(op1)
            op1 = op1 if vector else _scalar(op1)
            cmp = op0.Scale.Cmp(opOut.Scale)
            pre_scale = None
            if cmp == 0:
                if not vector and self.params.scheme._is_int(op1):
                    scale = Scale(1)
                else:
                    scale = pre_scale = Scale(self.params.Q()[level])
            elif cmp == -1:
                scale = opOut.Scale.Div(op0.Scale)
            else:
                raise ValueError("cannot MulThenAdd: op0.Scale > opOut.Scale is not supported")
            pre = None
            if pre_scale is not None:
                # Mul(opOut, scaleInt, opOut) (:959-964, :999-1003) runs at opOut's own level: the limbs above `level` are multiplied
                # here, those up to `level` inside the fused launch
                if opOut.Level() > level:
                    top = self._int_words(opOut.Level(), pre_scale.Int())
                    hi = self._ring(opOut.Level())
                    tmp = [Poly(self.params.ringQ, opOut.Level() + 1, opOut.batch, zero=False) for _ in opOut.Value]
                    for a, b in zip(opOut.Value, tmp):
                        b.CopyLvl(level, a)
                    ct_scalar(hi, 2, opOut.Value, top, top, opOut.Value)
                    for a, b in zip(opOut.Value, tmp):
                        a.CopyLvl(level, b)
                pre = self._int_words(level, pre_scale.Int())
                opOut.Scale = opOut.Scale.Mul(pre_scale)
            if vector:  # :1012-1025: encoded at scaleRLWE, then MulThenAdd with the plaintext (the scales now agree: no second scale-up)
                pt = self._encode(op1, level, op0.MetaData, scale, op0.batch)
                ct_mul_pt(self._ring(level), op0.Value, pt.Value[0], opOut.Value, then_add=True, pre=pre)
                return
            s0, s1 = self._scalar_words(level, scale, op1)
            ct_scalar(self._ring(level), 3, op0.Value, s0, s1, opOut.Value, pre=pre)
            return
        if not _is_element(op1):
            raise ValueError(_OPERAND_ERROR % type(op1).__name__)
        name = "MulThenAdd" if not relin else "MulRelinThenAdd"
        try:
            _, level = self.InitOutputBinaryOp(op0, op1, 2, opOut)
        except ValueError as e:
            raise ValueError(f"cannot {name}: {e}") from None
        if op0 is opOut or op1 is opOut:
            raise ValueError(f"cannot {name}: opOut must be different from op0 and op1")
        opOut.Resize(opOut.Degree(), level)
        # mulRelinThenAdd (:1081-1173)
        level = opOut.Level()
        res = op0.Scale.Mul(op1.Scale)
        pre = None
        if opOut.Scale.Cmp(res) == -1:
            ratio = res.Div(opOut.Scale)
            if ratio.Float64() >= 2.0:
                # Mul(opOut, &ratio.Value, opOut): a *big.Float operand -- an integer ratio multiplies as it is, any other one is
                # encoded at scale q_level, as the reference does (:1091)
                scale = Scale(1) if self.params.scheme._is_int(ratio.Value) else Scale(self.params.Q()[level])
                pre = self._scalar_words(level, scale, ratio.Value)[0]
                opOut.Scale = res
        if op0.Degree() == 1 and op1.Degree() == 1:
            if relin and self.rlk is None:  # (:1139-1141, wrapped by :1073)
                raise ValueError("cannot MulRelinThenAdd: cannot relinearize: EvaluationKeySet is nil")
            opOut.Resize(max(1, opOut.Degree()) if relin else 2, level)
            out = opOut.Value[:2] if relin else opOut.Value
            if relin and opOut.Degree() == 2 and pre is not None:  # (the scale-up acts on every component of opOut)
                ct_scalar(self._ring(level), 2, opOut.Value[2:], pre, pre, opOut.Value[2:])
            ct_mul_relin_then_add(self.ev, level, op0.Value, op1.Value, self.rlk if relin else None, out, pre=pre)
        else:
            if op0.Degree() == 0:
                raise ValueError(f"cannot {name}: op0 must be a ciphertext when op1 is a plaintext")
            opOut.Resize(max(op0.Degree(), opOut.Degree()), level)
            n = op0.Degree() + 1
            if pre is not None and opOut.Degree() + 1 > n:
                ct_scalar(self._ring(level), 2, opOut.Value[n:], pre, pre, opOut.Value[n:])
            ct_mul_pt(self._ring(level), op0.Value, op1.Value[0], opOut.Value[:n], then_add=True, pre=pre)

    def MulThenAdd(self, op0, op1, opOut):
        self._mul_then_add(op0, op1, opOut, False, "MulThenAdd")

    def MulRelinThenAdd(self, op0, op1, opOut):
        self._mul_then_add(op0, op1, opOut, True, "MulRelinThenAdd")

    # -- Relinearize, Rescale, SetScale, ScaleUp, DropLevel
    def Relinearize(self, op0, opOut):
        if op0.Degree() != 2:
            raise ValueError("cannot relinearize: element must be of degree 2")
        if self.rlk is None:
            raise ValueError("cannot relinearize: EvaluationKeySet is nil")
        level = min(op0.Level(), opOut.Level())
        opOut.Resize(max(1, opOut.Degree()), level)
        self.ev.Relinearize(level, op0.Value, self.rlk, opOut.Value[:2])
        opOut.Resize(1, level)
        opOut.MetaData = op0.MetaData.copy()

    def RelinearizeNew(self, op0):
        opOut = NewCiphertext(self.params, 1, op0.Level(), op0.batch)
        self.Relinearize(op0, opOut)
        return opOut

    def Rescale(self, op0, opOut):
        """Evaluator.Rescale (:477-521): one division by the last modulus; the scale is divided by it"""
        if op0.Level() == 0:
            raise ValueError("cannot Rescale: input Ciphertext already at level 0")
        if opOut.Degree() != op0.Degree():
            raise ValueError("cannot Rescale: op0.Degree() != opOut.Degree()")
        level = op0.Level()
        meta = op0.MetaData.copy()
        meta.Scale = op0.Scale.Div(self.params.Q()[level])
        if opOut is not op0:
            opOut.Resize(op0.Degree(), level)
        self.ev.Rescale(level, 1, op0.Value, opOut.Value)
        opOut.MetaData = meta
        opOut.Resize(op0.Degree(), level - 1)

    def RescaleNew(self, op0):
        opOut = NewCiphertext(self.params, op0.Degree(), op0.Level(), op0.batch)
        self.Rescale(op0, opOut)
        return opOut

    def ScaleUp(self, op0, scale, opOut):
        """:433-443: Mul(op0, scale.Uint64(), opOut); opOut.Scale = op0.Scale * scale"""
        from .rlwe import Scale
        self.Mul(op0, Scale(scale).Uint64(), opOut)
        opOut.Scale = op0.Scale.Mul(scale)

    def ScaleUpNew(self, op0, scale):
        opOut = NewCiphertext(self.params, op0.Degree(), op0.Level(), op0.batch)
        self.ScaleUp(op0, scale, opOut)
        return opOut

    def DropLevel(self, op0, levels: int):
        op0.Resize(op0.Degree(), op0.Level() - levels)

    def DropLevelNew(self, op0, levels: int):
        opOut = op0.CopyNew()
        self.DropLevel(opOut, levels)
        return opOut

    # -- RescaleTo, SetScale (:445-457, :523-585)
    def RescaleTo(self, op0, minScale, opOut):
        from .rlwe import Scale
        minScale = Scale(minScale)
        if minScale.Cmp(0) != 1:
            raise ValueError("cannot RescaleTo: minScale is <0")
        minScale = minScale.Div(2)
        if op0.Scale.Cmp(0) != 1:
            raise ValueError("cannot RescaleTo: ciphertext scale is <0")
        if op0.Level() == 0:
            raise ValueError("cannot RescaleTo: input Ciphertext already at level 0")
        meta, level, Q = op0.MetaData.copy(), op0.Level(), self.params.Q()
        newLevel, nb = level, 0
        while newLevel >= 0:
            scale = meta.Scale.Div(Q[newLevel])
            if scale.Cmp(minScale) == -1:
                break
            meta.Scale = scale
            nb += 1
            newLevel -= 1
        if nb > level:
            raise ValueError("cannot RescaleTo: the scale allows more divisions than the ciphertext has levels")
        if opOut is not op0:
            opOut.Resize(op0.Degree(), level)
        if nb > 0:
            self.ev.Rescale(level, nb, op0.Value, opOut.Value)
        elif opOut is not op0:
            for a, b in zip(opOut.Value, op0.Value):
                a.CopyLvl(level, b)
        opOut.MetaData = meta
        opOut.Resize(op0.Degree(), level - nb)

    def SetScale(self, ct, scale):
        """Mul(ct, &ratioFlo, ct) with ratio = scale / ct.Scale as a *big.Float -- an integer ratio multiplies as it is, any other one
        is encoded at scale q_level -- then RescaleTo(ct, scale, ct), and the scale is set"""
        from .rlwe import Scale
        scale = Scale(scale)
        self.Mul(ct, scale.Div(ct.Scale).Value, ct)
        self.RescaleTo(ct, scale, ct)
        ct.Scale = scale

    # -- the key-switching methods (:1183-1318), over lattigo_amd.rlwe.CKKSRotations / InnerSumEvaluator
    def _like(self, op0, degree=None):
        out = NewCiphertext(self.params, op0.Degree() if degree is None else degree, op0.Level(), op0.batch)
        return out

    def _unary(self, op0, opOut, name):
        if op0.Degree() != 1 or opOut.Degree() != 1:
            raise ValueError(f"cannot {name}: cannot apply Automorphism: input and output Ciphertext must be of degree 1")
        level = min(op0.Level(), opOut.Level())
        opOut.Resize(1, level)
        return level

    def ApplyEvaluationKey(self, op0, evk, opOut):
        level = self._unary(op0, opOut, "ApplyEvaluationKey")
        self.ev.ApplyEvaluationKey(level, op0.Value, evk, opOut.Value)
        opOut.MetaData = op0.MetaData.copy()

    def ApplyEvaluationKeyNew(self, op0, evk):
        opOut = self._like(op0)
        self.ApplyEvaluationKey(op0, evk, opOut)
        return opOut

    def Rotate(self, op0, k: int, opOut):
        rot = self._rotations("Rotate")
        level = self._unary(op0, opOut, "Rotate")
        try:
            rot.Rotate(level, op0.Value, k, opOut.Value)
        except KeyError as e:
            raise ValueError(f"cannot Rotate: cannot apply Automorphism: {e.args[0]}") from None
        opOut.MetaData = op0.MetaData.copy()

    def RotateNew(self, op0, k: int):
        opOut = self._like(op0)
        self.Rotate(op0, k, opOut)
        return opOut

    def Conjugate(self, op0, opOut):
        if getattr(self.params.ringQ, "conjugate_invariant", False):
            raise ValueError("cannot Conjugate: method is not supported when parameters.RingType() == ring.ConjugateInvariant")
        rot = self._rotations("Conjugate")
        level = self._unary(op0, opOut, "Conjugate")
        try:
            rot.Conjugate(level, op0.Value, opOut.Value)
        except KeyError as e:
            raise ValueError(f"cannot Conjugate: cannot apply Automorphism: {e.args[0]}") from None
        opOut.MetaData = op0.MetaData.copy()

    def ConjugateNew(self, op0):
        opOut = self._like(op0)
        self.Conjugate(op0, opOut)
        return opOut

    def RotateHoisted(self, ctIn, rotations, opOut: dict):
        rot = self._rotations("RotateHoisted")
        level = ctIn.Level()
        for i in rotations:
            opOut[i].Resize(1, level)
        try:
            rot.RotateHoisted(level, ctIn.Value, rotations, {i: opOut[i].Value for i in rotations})
        except KeyError as e:
            raise ValueError(f"cannot RotateHoisted: {e.args[0]}") from None
        for i in rotations:
            opOut[i].MetaData = ctIn.MetaData.copy()

    def RotateHoistedNew(self, ctIn, rotations) -> dict:
        opOut = {i: self._like(ctIn, 1) for i in rotations}
        self.RotateHoisted(ctIn, rotations, opOut)
        return opOut

    def RotateHoistedLazyNew(self, level: int, rotations, ct, c2DecompQP) -> dict:
        """-> {rotation: [(Q0, P0), (Q1, P1)]}, the elements over QP of the reference (no entry for rotation 0)"""
        try:
            return self._rotations("RotateHoistedLazyNew").RotateHoistedLazyNew(level, rotations, ct.Value, c2DecompQP)
        except KeyError as e:
            raise ValueError(f"cannot RotateHoistedLazyNew: {e.args[0]}") from None

    def InnerSum(self, ctIn, batchSize: int, n: int, opOut):
        rot = self._rotations("InnerSum")
        level = self._unary(ctIn, opOut, "InnerSum")
        rot.InnerSum(level, ctIn.Value, batchSize, n, opOut.Value, slots=1 << ctIn.LogDimensions[1])
        opOut.MetaData = ctIn.MetaData.copy()

    def RotateAndAdd(self, ctIn, batchSize: int, n: int, opOut):
        rot = self._rotations("RotateAndAdd")
        level = self._unary(ctIn, opOut, "RotateAndAdd")
        rot.ise.PartialTracesSum(level, ctIn.Value, batchSize, n, opOut.Value)
        opOut.MetaData = ctIn.MetaData.copy()


# ---- converters from the element classes of lattigo_amd.encryptor and lattigo_amd.polyeval --------------------------------------------
def FromPolys(params: Parameters, Value, level: int, Scale_, *, LogSlots: int | None = None, IsBatched: bool = True):
    """a Ciphertext (two or three polynomials) or Plaintext (one) over existing device polynomials -- what lattigo_amd.encryptor's
    Encrypt fills and what lattigo_amd.polyeval.Ciphertext holds (its .Value, .level and .Scale); the polynomials are shared"""
    from .rlwe import Ciphertext, MetaData, Plaintext
    Value = list(Value)
    ls = params.ringQ.N.bit_length() - 2 if LogSlots is None else LogSlots
    meta = MetaData(Scale_, True, False, IsBatched, (0, ls))
    if len(Value) == 1:
        return Plaintext(params.ringQ, level, Value[0].batch, Value=Value, MetaData_=meta)
    return Ciphertext(params.ringQ, len(Value) - 1, level, Value[0].batch, Value=Value, MetaData_=meta)


def FromPolyEval(params: Parameters, ct, **kw):
    """lattigo_amd.polyeval.Ciphertext -> rlwe.Ciphertext (its rational scale rounded to 128 bits)"""
    return FromPolys(params, ct.Value, ct.level, ct.Scale, **kw)
