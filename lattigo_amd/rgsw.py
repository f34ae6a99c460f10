"""Host-side mirror of core/rgsw (elements.go, evaluator.go): the RGSW ciphertext as two device-resident gadget ciphertexts and
the external product RLWE x RGSW -> RLWE, backed by include/hering_rgsw.h.  A ciphertext is a list of two ``Poly``
(rlwe.Ciphertext.Value), NTT domain."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import encryptor as _enc
from . import rlwe, wire
from ._lib import H, check, load


class Ciphertext:
    """rgsw.Ciphertext (core/rgsw/elements.go:12): Value [2]rlwe.GadgetCiphertext, here two EvaluationKeys of one evaluator and
    one shape."""

    def __init__(self, value0: rlwe.EvaluationKey, value1: rlwe.EvaluationKey):
        if value0.Shape() != value1.Shape():
            raise ValueError("rgsw.Ciphertext: the two gadget ciphertexts differ in shape")
        self.Value = [value0, value1]

    def LevelQ(self) -> int:
        return self.Value[0].LevelQ()

    def LevelP(self) -> int:
        return self.Value[0].LevelP()

    def MarshalBinary(self) -> bytes:
        """rgsw.Ciphertext.MarshalBinary (elements.go:98): the two gadget ciphertexts back to back"""
        parts = []
        for k in self.Value:
            w = k.download()
            parts.append((w[:, :, : k.nQk], w[:, :, k.nQk:], k.BaseTwoDecomposition, k.BaseTwoDecompositionVectorSize))
        return wire.rgsw_ciphertext_marshal(*parts)


class KeySet:
    """A table of RGSW ciphertexts of one shape resident on the device (BlindRotationEvaluationKeySet's keys,
    core/rgsw/blindrot/keys.go), addressed by index from ExternalProductSelect."""

    def __init__(self, evaluator: "Evaluator", keys):
        self.keys = list(keys)
        n = len(self.keys)
        a0 = (H * n)(*[k.Value[0].h for k in self.keys])
        a1 = (H * n)(*[k.Value[1].h for k in self.keys])
        h = H()
        check(load().he_rgsw_keyset_create(evaluator.h, n, a0, a1, C.byref(h)))
        self.h = h.value

    def __len__(self):
        return len(self.keys)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                load().he_rgsw_keyset_destroy(self.h)
                self.h = None
        except Exception:
            pass


class Evaluator(rlwe.Evaluator):
    """rgsw.Evaluator (core/rgsw/evaluator.go:14): an rlwe.Evaluator with the external product."""

    def NewCiphertext(self, q0, p0, q1, p1, BaseTwoDecomposition=0, BaseTwoDecompositionVectorSize=None) -> Ciphertext:
        return Ciphertext(self.NewEvaluationKey(q0, p0, BaseTwoDecomposition, BaseTwoDecompositionVectorSize),
                          self.NewEvaluationKey(q1, p1, BaseTwoDecomposition, BaseTwoDecompositionVectorSize))

    def CiphertextFromBinary(self, data: bytes) -> Ciphertext:
        """rgsw.Ciphertext.UnmarshalBinary (elements.go:106) onto the device"""
        (q0, p0, b0, nj0), (q1, p1, b1, nj1) = wire.rgsw_ciphertext_unmarshal(data)
        if b0 != b1:
            raise ValueError("rgsw.Ciphertext: the two gadget ciphertexts differ in BaseTwoDecomposition")
        return Ciphertext(self.NewEvaluationKey(q0, p0 if p0.shape[2] else None, b0, nj0 if b0 else None),
                          self.NewEvaluationKey(q1, p1 if p1.shape[2] else None, b1, nj1 if b1 else None))

    def NewKeySet(self, keys) -> KeySet:
        return KeySet(self, keys)

    def ExternalProduct(self, op0, op1: Ciphertext, opOut):
        """ExternalProduct (:39): opOut = (<op0, op1[0]>, <op0, op1[1]>); opOut may be op0.  Levels are those of op1."""
        check(load().he_rgsw_external_product(self.h, op0[0].h, op0[1].h, op1.Value[0].h, op1.Value[1].h, opOut[0].h, opOut[1].h))

    def ExternalProductSelect(self, op0, keys: KeySet, sel, opOut):
        """Batch entry b of op0 times keys[sel[b]]; sel[b] == -1 passes the entry through.  One launch, small rings only."""
        s = np.ascontiguousarray(sel, dtype=np.int32)
        check(load().he_rgsw_external_product_select(self.h, op0[0].h, op0[1].h, keys.h, s.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     int(s.size), opOut[0].h, opOut[1].h))


# ---- rgsw.Encryptor (core/rgsw/encryptor.go; include/hering_rgsw_encryptor.h) ---------------------------------------------------
def NewCiphertext(evaluator: rlwe.Evaluator, levelQ: int, levelP: int, BaseTwoDecomposition: int = 0) -> Ciphertext:
    """rgsw.NewCiphertext (elements.go:27): a zeroed ciphertext at (levelQ, levelP, BaseTwoDecomposition)"""
    from .keygen import BaseTwoDecompositionVectorSize

    def key():
        if BaseTwoDecomposition:
            nj = BaseTwoDecompositionVectorSize(evaluator.ringQ.moduli, levelQ, levelP, BaseTwoDecomposition)
            return rlwe.EvaluationKey(evaluator, None, None, BaseTwoDecomposition, nj, shape=(sum(nj), levelQ + 1, levelP + 1))
        return rlwe.EvaluationKey(evaluator, None, None, shape=(rlwe.BaseRNSDecompositionVectorSize(levelQ, levelP), levelQ + 1, levelP + 1))
    return Ciphertext(key(), key())


class Encryptor(_enc.Encryptor):
    """rgsw.NewEncryptor(params, key): an rlwe.Encryptor whose Encrypt and EncryptZero also take an rgsw.Ciphertext (secret-key
    encryption only).  Every call is an exact function of the byte stream of the PRNG; the drawing order is the reference's: per
    row (i, j) one encryptZeroSk on Value[0][i][j], then one on Value[1][i][j]; in a table, ciphertext after ciphertext."""

    def __init__(self, evaluator: rlwe.Evaluator, prng, sk=None, XeSigma: float = _enc.DefaultXeSigma, XeBound: float = _enc.DefaultXeBound):
        super().__init__(evaluator, prng, sk, _enc.DefaultXsP, XeSigma, XeBound)

    def EncryptZero(self, ct):
        if not isinstance(ct, Ciphertext):
            return super().EncryptZero(ct)
        self.prng.check(load().he_rgsw_encrypt_zero(self.h, ct.Value[0].h, ct.Value[1].h))

    def Encrypt(self, pt, ct):
        """pt: an rlwe Plaintext (Value, IsNTT, IsMontgomery) or None"""
        if not isinstance(ct, Ciphertext):
            return super().Encrypt(pt, ct)
        if pt is None:
            return self.EncryptZero(ct)
        self.prng.check(load().he_rgsw_encrypt(self.h, pt.Value.h, int(pt.IsNTT), int(pt.IsMontgomery), ct.Value[0].h, ct.Value[1].h))

    def EncryptTable(self, pts, sel, cts):
        """cts[k] = Encrypt(entry sel[k] of pts) for k = 0, 1, ... on the one source; pts: one Poly of batch m (NTT and Montgomery)
        or None; sel[k] == -1: EncryptZero.  One finishing launch per chunk of ciphertexts."""
        s = np.ascontiguousarray(sel, dtype=np.int32)
        n = len(cts)
        if s.size != n:
            raise ValueError("sel and cts must have the same length")
        a0 = (H * max(n, 1))(*[c.Value[0].h for c in cts])
        a1 = (H * max(n, 1))(*[c.Value[1].h for c in cts])
        self.prng.check(load().he_rgsw_encrypt_table(self.h, pts.h if pts is not None else 0, s.ctypes.data_as(C.POINTER(C.c_int32)), n, a0, a1))


# ---- the element-wise helpers of core/rgsw/evaluator.go:283-356, on the device words of the keys -----------------------------
# ringQP is accepted for the reference's argument order and not used: the keys carry their evaluator's rings.
ADD_LAZY, REDUCE, MUL_LAZY, MUL_THEN_ADD_LAZY = 0, 1, 2, 3


class Plaintext:
    """rgsw.Plaintext = rlwe.GadgetPlaintext (core/rlwe/gadgetciphertext.go:325): Value []ring.Poly, one polynomial per window
    2^(j BaseTwoDecomposition), NTT + Montgomery -- here one Poly over the Q moduli whose batch entry j is Value[j]."""

    def __init__(self, value):
        self.Value = value


def _key_op(op, ctIn: Ciphertext, powXMinusOne, opOut: Ciphertext):
    xQ, xP = (powXMinusOne[0].h, powXMinusOne[1].h if powXMinusOne[1] is not None else 0) if powXMinusOne is not None else (0, 0)
    for k in range(2):
        check(load().he_rgsw_key_op(op, ctIn.Value[k].h, xQ, xP, opOut.Value[k].h))


def AddLazy(op, ringQP, opOut: Ciphertext):
    """AddLazy (:283): opOut += op without modular reduction; op a Plaintext or a Ciphertext"""
    if isinstance(op, Plaintext):
        check(load().he_rgsw_key_add_plaintext_lazy(op.Value.h, opOut.Value[0].h, opOut.Value[1].h))
    elif isinstance(op, Ciphertext):
        _key_op(ADD_LAZY, op, None, opOut)
    else:
        raise TypeError("cannot AddLazy: unsuported op.(type), must be either *rgsw.Plaintext or *rgsw.Ciphertext")


def Reduce(ctIn: Ciphertext, ringQP, opOut: Ciphertext):
    """Reduce (:323): opOut = ctIn mod q, canonical words"""
    _key_op(REDUCE, ctIn, None, opOut)


def MulByXPowAlphaMinusOneLazy(ctIn: Ciphertext, powXMinusOne, ringQP, opOut: Ciphertext):
    """MulByXPowAlphaMinusOneLazy (:335): opOut = ctIn * powXMinusOne, every row; powXMinusOne = (Q, P) polynomials of X^alpha - 1
    (P is None without special primes), NTT + Montgomery; lazy words in [0, 2q)"""
    _key_op(MUL_LAZY, ctIn, powXMinusOne, opOut)


def MulByXPowAlphaMinusOneThenAddLazy(ctIn: Ciphertext, powXMinusOne, ringQP, opOut: Ciphertext):
    """MulByXPowAlphaMinusOneThenAddLazy (:347): opOut += ctIn * powXMinusOne without reduction"""
    _key_op(MUL_THEN_ADD_LAZY, ctIn, powXMinusOne, opOut)
