"""rlwe.Encryptor, rlwe.Decryptor and KeyGenerator.GenPublicKey on the device (include/hering_encryptor.h; core/rlwe/encryptor.go,
decryptor.go, keygenerator.go:80-88).  Every call is an exact function of the byte stream of the encryptor's PRNG: the words, the
drawing order and the position of the source afterwards are the reference's (for a batch: step by step over the entries)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

from ._lib import H, check, load
from .ring import Poly
from .rlwe import Evaluator
from .sampling import PRNG

# the reference's defaults (core/rlwe/security.go): Xs = Ternary{P: 2/3}, Xe = DiscreteGaussian{Sigma: 3.2, Bound: 19.2}
DefaultXsP, DefaultXeSigma, DefaultXeBound = 2 / 3, 3.2, 19.2


@dataclass
class SecretKey:
    """rlwe.SecretKey: Value = ringqp.Poly{Q, P} in the NTT domain and Montgomery form (P None without special primes); the
    polynomials carry the batch of the ciphertexts they serve"""
    Q: Poly
    P: Poly | None = None


@dataclass
class PublicKey:
    """rlwe.PublicKey: Value[0], Value[1] as (Q, P) pairs, NTT and Montgomery"""
    Value: tuple


@dataclass
class Element:
    """rlwe.Element[ring.Poly] of degree len(Value) - 1 with the metadata the encryptor reads; Level() is its limbs in use"""
    Value: list
    IsNTT: bool = True
    IsMontgomery: bool = False
    level: int | None = None

    def Level(self):
        return self.Value[0].Level() if self.level is None else self.level

    def Degree(self):
        return len(self.Value) - 1


@dataclass
class ElementQP:
    """rlwe.Element[ringqp.Poly] of degree 1: Value[k] = (Q, P)"""
    Value: list
    IsNTT: bool = True
    IsMontgomery: bool = True
    levelQ: int | None = None
    levelP: int | None = None

    def LevelQ(self):
        return self.Value[0][0].Level() if self.levelQ is None else self.levelQ

    def LevelP(self):
        return self.Value[0][1].Level() if self.levelP is None else self.levelP


@dataclass
class Plaintext:
    """rlwe.Plaintext: Value with IsNTT / IsMontgomery"""
    Value: Poly
    IsNTT: bool = True
    IsMontgomery: bool = False
    level: int | None = None

    def Level(self):
        return self.Value.Level() if self.level is None else self.level


def _h(p):
    return p.h if p is not None else 0


class Encryptor:
    """rlwe.NewEncryptor(params, key) over the rings of `evaluator`"""

    def __init__(self, evaluator: Evaluator, prng: PRNG, key=None, XsP: float = DefaultXsP, XeSigma: float = DefaultXeSigma,
                 XeBound: float = DefaultXeBound):
        self.evaluator, self.prng, self.Xs, self.Xe = evaluator, prng, XsP, (XeSigma, XeBound)
        h = H()
        check(load().he_encryptor_create(evaluator.h, prng.h, float(XsP), float(XeSigma), float(XeBound), C.byref(h)))
        self.h = h.value
        self.key = None
        self._bind(key)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                load().he_encryptor_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def _bind(self, key):
        arr = (C.c_uint64 * 4)()
        if key is None:
            kind = 0
        elif isinstance(key, SecretKey):
            kind, arr[0], arr[1] = 1, _h(key.Q), _h(key.P)
        elif isinstance(key, PublicKey):
            kind = 2
            arr[0], arr[1], arr[2], arr[3] = _h(key.Value[0][0]), _h(key.Value[0][1]), _h(key.Value[1][0]), _h(key.Value[1][1])
        else:
            raise TypeError(f"invalid key type, want SecretKey, PublicKey or None but have {type(key)}")
        check(load().he_encryptor_set_key(self.h, kind, arr))
        self.key = key

    def WithKey(self, key) -> "Encryptor":
        """a shallow copy bound to `key` (sharing the evaluator's tables and the source)"""
        return Encryptor(self.evaluator, self.prng, key if key is not None else self.key, self.Xs, *self.Xe)

    def EncryptZero(self, ct):
        if isinstance(ct, ElementQP):
            (c0Q, c0P), (c1Q, c1P) = ct.Value
            levelP = -1 if c0P is None else ct.LevelP()  # (no special primes: a ringqp.Poly without a P part)
            self.prng.check(load().he_encrypt_zero_qp(self.h, ct.LevelQ(), levelP, int(ct.IsNTT), int(ct.IsMontgomery), c0Q.h, _h(c0P), c1Q.h, _h(c1P)))
        else:
            self.prng.check(load().he_encrypt_zero(self.h, ct.Level(), int(ct.IsNTT), int(ct.IsMontgomery), ct.Value[0].h, ct.Value[1].h))

    def Encrypt(self, pt: Plaintext | None, ct: Element):
        if pt is None:
            return self.EncryptZero(ct)
        level = C.c_int()
        self.prng.check(load().he_encrypt(self.h, pt.Level(), ct.Level(), int(pt.IsNTT), int(pt.IsMontgomery), pt.Value.h, ct.Value[0].h, ct.Value[1].h,
                                     C.byref(level)))
        ct.IsNTT, ct.IsMontgomery, ct.level = pt.IsNTT, pt.IsMontgomery, level.value  # *ct.MetaData = *pt.MetaData; ct.Resize

    def addPtToCt(self, level: int, pt: Plaintext, ct: Element):
        check(load().he_add_pt_to_ct(self.h, level, int(pt.IsNTT), int(ct.IsNTT), pt.Value.h, ct.Value[0].h))


class Decryptor:
    """rlwe.NewDecryptor(params, sk)"""

    def __init__(self, evaluator: Evaluator, sk: SecretKey):
        self.evaluator, self.sk = evaluator, sk
        h = H()
        check(load().he_decryptor_create(evaluator.h, sk.Q.h, C.byref(h)))
        self.h = h.value

    def __del__(self):
        try:
            if getattr(self, "h", None):
                load().he_decryptor_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def WithKey(self, sk: SecretKey) -> "Decryptor":
        return Decryptor(self.evaluator, sk)

    def Decrypt(self, ct: Element, pt: Plaintext):
        arr = (C.c_uint64 * len(ct.Value))(*[p.h for p in ct.Value])
        level = C.c_int()
        check(load().he_decryptor_decrypt(self.h, ct.Level(), pt.Level(), int(ct.IsNTT), ct.Degree(), arr, pt.Value.h, C.byref(level)))
        pt.IsNTT, pt.IsMontgomery, pt.level = ct.IsNTT, ct.IsMontgomery, level.value  # *pt.MetaData = *ct.MetaData; pt.Resize


class KeyGenerator:
    """rlwe.KeyGenerator restricted to GenPublicKey (keygenerator.go:80-88): an Encryptor under sk"""

    def __init__(self, evaluator: Evaluator, prng: PRNG, XsP: float = DefaultXsP, XeSigma: float = DefaultXeSigma, XeBound: float = DefaultXeBound):
        self.evaluator, self.prng, self.dist = evaluator, prng, (XsP, XeSigma, XeBound)

    def GenPublicKey(self, sk: SecretKey, pk: PublicKey):
        """pk: EncryptZero of the QP element (pk.Value) with IsNTT = IsMontgomery = true"""
        Encryptor(self.evaluator, self.prng, sk, *self.dist).EncryptZero(ElementQP([pk.Value[0], pk.Value[1]], True, True))

    def GenPublicKeyNew(self, sk: SecretKey) -> PublicKey:
        rq, rp, B = self.evaluator.ringQ, self.evaluator.ringP, sk.Q.batch
        pk = PublicKey(tuple((rq.NewPoly(B), rp.NewPoly(B) if rp is not None else None) for _ in range(2)))
        self.GenPublicKey(sk, pk)
        return pk
