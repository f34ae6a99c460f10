"""The threshold protocols of the reference's multiparty package on the device (include/hering_multiparty.h): PublicKeyGenProtocol
(multiparty/keygen_cpk.go), EvaluationKeyGenProtocol (keygen_evk.go), GaloisKeyGenProtocol (keygen_gal.go),
RelinearizationKeyGenProtocol (keygen_relin.go) and KeySwitchProtocol (keyswitch_sk.go), with the reference's method names and
argument order, and PublicKeySwitchProtocol (keyswitch_pk.go).  A protocol object is a party's view: it draws its Gaussians from the source
of the rlwe KeyGenerator it was made with; a CRS is any sampling.PRNG.  Every call is an exact function of the byte streams it reads.

CRPs and shares are device-resident (each wraps an EvaluationKey handle: a CRP lives in component 1, a share in component 0) and
marshal to the reference's wire form through lattigo_amd.wire."""
from __future__ import annotations

import math
import struct

import numpy as np

from . import wire
from ._lib import check, load
from .encryptor import Element, Encryptor, PublicKey, SecretKey, _h
from .keygen import EvaluationKeyParameters, GaloisKey, KeyGenerator
from .ring import Poly
from .rlwe import EvaluationKey
from .sampling import PRNG, UniformSampler


class _Gadget:
    """a gadget-shaped object of the protocols, on the handle of an EvaluationKey"""
    _comp, _comps = 0, 1

    def __init__(self, key: EvaluationKey):
        self.key = key

    def LevelQ(self):
        return self.key.LevelQ()

    def LevelP(self):
        return self.key.LevelP()

    def BaseRNSDecompositionVectorSize(self):
        nj = self.key.BaseTwoDecompositionVectorSize
        return len(nj) if nj else self.key.beta

    def BaseTwoDecompositionVectorSize(self):
        return list(self.key.BaseTwoDecompositionVectorSize or [1] * self.key.beta)

    def download(self) -> np.ndarray:
        """[rows][nQk + nPk][N]: the component this object lives in"""
        return self.key.download()[:, self._comp]

    def _parts(self):
        img = self.key.download()[:, self._comp:self._comp + self._comps]
        return img[:, :, :self.key.nQk], img[:, :, self.key.nQk:]

    def BinarySize(self) -> int:
        return wire.gadget_ciphertext_binary_size(self.BaseTwoDecompositionVectorSize(), self.key.nQk, self.key.nPk, self.key.N, self._comps)

    def MarshalBinary(self) -> bytes:
        q, p = self._parts()
        return wire.gadget_ciphertext_marshal(q, p, self.key.BaseTwoDecomposition, self.key.BaseTwoDecompositionVectorSize)


class EvaluationKeyGenCRP(_Gadget):
    """multiparty.EvaluationKeyGenCRP: Value[i][j] in component 1 of row (i, j)"""
    _comp = 1


class EvaluationKeyGenShare(_Gadget):
    """multiparty.EvaluationKeyGenShare: a GadgetCiphertext of degree 0"""


class GaloisKeyGenCRP(EvaluationKeyGenCRP):
    pass


class GaloisKeyGenShare(EvaluationKeyGenShare):
    """multiparty.GaloisKeyGenShare: the share with its Galois element, which leads its wire form (keygen_gal.go:95-133)"""

    def __init__(self, key: EvaluationKey, GaloisElement: int = 0):
        super().__init__(key)
        self.GaloisElement = int(GaloisElement)

    def BinarySize(self) -> int:
        return 8 + super().BinarySize()

    def MarshalBinary(self) -> bytes:
        return struct.pack("<Q", self.GaloisElement) + super().MarshalBinary()


class EvaluationKeyGenProtocol:
    """multiparty.NewEvaluationKeyGenProtocol(params): `kgen` stands for the parameters, the party's source and its Xe"""
    _CRP, _Share = EvaluationKeyGenCRP, EvaluationKeyGenShare

    def __init__(self, kgen: KeyGenerator):
        self.kgen = kgen

    def ShallowCopy(self, kgen: KeyGenerator) -> "EvaluationKeyGenProtocol":
        """a view for another party (the reference forks the party's PRNG; here the other party's generator is given)"""
        return type(self)(kgen)

    def AllocateShare(self, evkParams: EvaluationKeyParameters | None = None):
        return self._Share(self.kgen.NewEvaluationKey(evkParams))

    def SampleCRP(self, crs: PRNG, evkParams: EvaluationKeyParameters | None = None):
        crp = self._CRP(self.kgen.NewEvaluationKey(evkParams))
        crs.check(load().he_mp_crp_gadget(self.kgen.evaluator.h, crs.h, crp.key.h))
        return crp

    def GenShare(self, skIn: SecretKey, skOut: SecretKey, crp: EvaluationKeyGenCRP, shareOut: EvaluationKeyGenShare):
        self.kgen.prng.check(load().he_mp_evk_gen_share(self.kgen.h, skIn.Q.h, skOut.Q.h, _h(skOut.P), crp.key.h, shareOut.key.h))

    def AggregateShares(self, share1, share2, share3):
        check(load().he_mp_gadget_aggregate(share1.key.h, share2.key.h, 0, share3.key.h))

    def GenEvaluationKey(self, share: EvaluationKeyGenShare, crp: EvaluationKeyGenCRP, evk: EvaluationKey):
        check(load().he_mp_evk_finalize(share.key.h, crp.key.h, evk.h))


class GaloisKeyGenProtocol(EvaluationKeyGenProtocol):
    """multiparty.NewGaloisKeyGenProtocol(params)"""
    _CRP, _Share = GaloisKeyGenCRP, GaloisKeyGenShare

    def GenShare(self, sk: SecretKey, galEl: int, crp: GaloisKeyGenCRP, shareOut: GaloisKeyGenShare):
        self.kgen.prng.check(load().he_mp_galois_gen_share(self.kgen.h, int(galEl), sk.Q.h, _h(sk.P), crp.key.h, shareOut.key.h))
        shareOut.GaloisElement = int(galEl)  # "Important" (keygen_gal.go:60)

    def AggregateShares(self, share1: GaloisKeyGenShare, share2: GaloisKeyGenShare, share3: GaloisKeyGenShare):
        if share1.GaloisElement != share2.GaloisElement:
            raise ValueError(f"cannot aggregate: GaloisKeyGenShares do not share the same GaloisElement: {share1.GaloisElement} != {share2.GaloisElement}")
        share3.GaloisElement = share1.GaloisElement
        super().AggregateShares(share1, share2, share3)

    def GenGaloisKey(self, share: GaloisKeyGenShare, crp: GaloisKeyGenCRP, gk: GaloisKey):
        self.GenEvaluationKey(share, crp, gk.EvaluationKey)
        gk.GaloisElement, gk.NthRoot = share.GaloisElement, self.kgen.evaluator.ringQ.NthRoot()


class RelinearizationKeyGenCRP(EvaluationKeyGenCRP):
    pass


class RelinearizationKeyGenShare(_Gadget):
    """multiparty.RelinearizationKeyGenShare: a GadgetCiphertext of degree 1 (round one) or 0 (round two)"""

    def __init__(self, key: EvaluationKey, degree: int):
        super().__init__(key)
        self._comps = int(degree) + 1

    def Degree(self):
        return self._comps - 1

    def download(self) -> np.ndarray:
        """[rows][degree + 1][nQk + nPk][N]"""
        return self.key.download()[:, :self._comps]


class RelinearizationKeyGenProtocol:
    """multiparty.NewRelinearizationKeyGenProtocol(params): the party's ternary and Gaussian samplers read the generator's source"""

    def __init__(self, kgen: KeyGenerator):
        self.kgen = kgen

    def SampleCRP(self, crs: PRNG, evkParams: EvaluationKeyParameters | None = None) -> RelinearizationKeyGenCRP:
        crp = RelinearizationKeyGenCRP(self.kgen.NewEvaluationKey(evkParams))
        crs.check(load().he_mp_crp_gadget(self.kgen.evaluator.h, crs.h, crp.key.h))
        return crp

    def AllocateShare(self, evkParams: EvaluationKeyParameters | None = None):
        """(ephSk, r1, r2): the ephemeral key at the parameters' top levels, a degree-1 and a degree-0 share"""
        rq, rp = self.kgen.evaluator.ringQ, self.kgen.evaluator.ringP
        eph = SecretKey(rq.NewPoly(), rp.NewPoly() if rp is not None else None)
        return (eph, RelinearizationKeyGenShare(self.kgen.NewEvaluationKey(evkParams), 1),
                RelinearizationKeyGenShare(self.kgen.NewEvaluationKey(evkParams), 0))

    def GenShareRoundOne(self, sk: SecretKey, crp: RelinearizationKeyGenCRP, ephSkOut: SecretKey, shareOut: RelinearizationKeyGenShare):
        self.kgen.prng.check(load().he_mp_rkg_round_one(self.kgen.h, sk.Q.h, _h(sk.P), crp.key.h, ephSkOut.Q.h, _h(ephSkOut.P), shareOut.key.h))

    def GenShareRoundTwo(self, ephSk: SecretKey, sk: SecretKey, round1: RelinearizationKeyGenShare, shareOut: RelinearizationKeyGenShare):
        self.kgen.prng.check(load().he_mp_rkg_round_two(self.kgen.h, ephSk.Q.h, _h(ephSk.P), sk.Q.h, _h(sk.P), round1.key.h, shareOut.key.h))

    def AggregateShares(self, share1: RelinearizationKeyGenShare, share2: RelinearizationKeyGenShare, shareOut: RelinearizationKeyGenShare):
        check(load().he_mp_gadget_aggregate(share1.key.h, share2.key.h, share1.Degree(), shareOut.key.h))

    def GenRelinearizationKey(self, round1: RelinearizationKeyGenShare, round2: RelinearizationKeyGenShare, evalKeyOut: EvaluationKey):
        check(load().he_mp_rlk_finalize(round1.key.h, round2.key.h, evalKeyOut.h))


class _PolyQP:
    """a ringqp.Poly of the protocols: (Q, P), P None without special primes"""

    def __init__(self, Q: Poly, P: Poly | None):
        self.Q, self.P = Q, P

    def BinarySize(self) -> int:
        return wire.poly_binary_size(self.Q.n_limbs, self.Q.N) + wire.poly_binary_size(self.P.n_limbs if self.P is not None else 0, self.Q.N)

    def MarshalBinary(self) -> bytes:
        p = self.P.download()[0] if self.P is not None else np.zeros((0, self.Q.N), dtype=np.uint64)
        return wire.polyqp_marshal(self.Q.download()[0], p)


class PublicKeyGenCRP(_PolyQP):
    pass


class PublicKeyGenShare(_PolyQP):
    pass


class PublicKeyGenProtocol:
    """multiparty.NewPublicKeyGenProtocol(params)"""

    def __init__(self, kgen: KeyGenerator):
        self.kgen = kgen

    def _new(self, cls):
        rq, rp = self.kgen.evaluator.ringQ, self.kgen.evaluator.ringP
        return cls(rq.NewPoly(), rp.NewPoly() if rp is not None else None)

    def AllocateShare(self) -> PublicKeyGenShare:
        return self._new(PublicKeyGenShare)

    def SampleCRP(self, crs: PRNG) -> PublicKeyGenCRP:
        crp = self._new(PublicKeyGenCRP)
        ev = self.kgen.evaluator
        UniformSampler(crs, ev.ringQ, ev.ringP).Read(crp.Q if crp.P is None else (crp.Q, crp.P))
        return crp

    def GenShare(self, sk: SecretKey, crp: PublicKeyGenCRP, shareOut: PublicKeyGenShare):
        self.kgen.prng.check(load().he_mp_pk_gen_share(self.kgen.h, sk.Q.h, _h(sk.P), crp.Q.h, _h(crp.P), shareOut.Q.h, _h(shareOut.P)))

    def AggregateShares(self, share1: PublicKeyGenShare, share2: PublicKeyGenShare, shareOut: PublicKeyGenShare):
        ev = self.kgen.evaluator
        check(load().he_add(ev.ringQ.h, ev.ringQ.MaxLevel(), share1.Q.h, share2.Q.h, shareOut.Q.h))
        if shareOut.P is not None:
            check(load().he_add(ev.ringP.h, ev.ringP.MaxLevel(), share1.P.h, share2.P.h, shareOut.P.h))

    def GenPublicKey(self, roundShare: PublicKeyGenShare, crp: PublicKeyGenCRP, pubkey: PublicKey):
        for dst, src in zip(pubkey.Value, (roundShare, crp)):
            check(load().he_poly_copy(dst[0].h, src.Q.h, src.Q.n_limbs - 1))
            if src.P is not None:
                check(load().he_poly_copy(dst[1].h, src.P.h, src.P.n_limbs - 1))


class KeySwitchCRP:
    def __init__(self, Value: Poly):
        self.Value = Value


class KeySwitchShare:
    """multiparty.KeySwitchShare: one polynomial, words in [0, 2q)"""

    def __init__(self, Value: Poly):
        self.Value = Value

    def Level(self):
        return self.Value.n_limbs - 1

    def BinarySize(self) -> int:
        return wire.poly_binary_size(self.Value.n_limbs, self.Value.N)

    def MarshalBinary(self) -> bytes:
        return wire.poly_marshal(self.Value.download()[0])


class KeySwitchProtocol:
    """multiparty.NewKeySwitchProtocol(params, noiseFlooding = DiscreteGaussian{Sigma: noiseSigma}): the noise is
    DiscreteGaussian{sqrt(NoiseFreshSK^2 + noiseSigma^2), 6 sigma} (keyswitch_sk.go:49-52), read from the generator's source.
    NoiseFreshSK is the parameters' Xe.Sigma (core/rlwe/params.go)"""

    def __init__(self, kgen: KeyGenerator, noiseSigma: float, NoiseFreshSK: float):
        self.kgen = kgen
        self.Sigma = math.sqrt(float(NoiseFreshSK) ** 2 + float(noiseSigma) ** 2)
        self.Bound = 6 * self.Sigma

    def AllocateShare(self, level: int) -> KeySwitchShare:
        return KeySwitchShare(self.kgen.evaluator.ringQ.AtLevel(level).NewPoly())

    def SampleCRP(self, level: int, crs: PRNG) -> KeySwitchCRP:
        rq = self.kgen.evaluator.ringQ.AtLevel(level)
        crp = rq.NewPoly()
        UniformSampler(crs, rq).Read(crp)
        return KeySwitchCRP(crp)

    def GenShare(self, skInput: SecretKey, skOutput: SecretKey, ct: Element, shareOut: KeySwitchShare):
        level = min(shareOut.Level(), ct.Value[1].n_limbs - 1)  # :84
        self.kgen.prng.check(load().he_mp_cks_gen_share(self.kgen.h, level, skInput.Q.h, skOutput.Q.h, ct.Value[1].h, int(ct.IsNTT), self.Sigma,
                                                        self.Bound, shareOut.Value.h))

    def AggregateShares(self, share1: KeySwitchShare, share2: KeySwitchShare, shareOut: KeySwitchShare):
        if not share1.Level() == share2.Level() == shareOut.Level():
            raise ValueError("cannot AggregateShares: shares levels do not match")
        check(load().he_add(self.kgen.evaluator.ringQ.h, share1.Level(), share1.Value.h, share2.Value.h, shareOut.Value.h))

    def KeySwitch(self, ctIn: Element, combined: KeySwitchShare, opOut: Element):
        level = ctIn.Value[0].n_limbs - 1
        if ctIn is not opOut:
            check(load().he_poly_copy(opOut.Value[1].h, ctIn.Value[1].h, level))
            opOut.IsNTT, opOut.IsMontgomery = ctIn.IsNTT, ctIn.IsMontgomery
        check(load().he_add(self.kgen.evaluator.ringQ.h, level, ctIn.Value[0].h, combined.Value.h, opOut.Value[0].h))


class PublicKeySwitchShare:
    """multiparty.PublicKeySwitchShare: an rlwe.Element of degree 1 with the MetaData rlwe.NewElement gives it (core/rlwe/element.go:
    38-52: the zero PlaintextMetaData and IsNTT = the parameters' NTTFlag), which GenShare does not change and the wire form carries"""

    def __init__(self, Value, IsNTT: bool = True):
        self.Value = list(Value)
        self.IsNTT = bool(IsNTT)

    def Level(self):
        return self.Value[0].n_limbs - 1

    def BinarySize(self) -> int:
        """Element.BinarySize (element.go:315-322): the flag byte, the MetaData, the vector of polynomials"""
        return 1 + wire.METADATA_BINARY_SIZE + 8 + 2 * wire.poly_binary_size(self.Value[0].n_limbs, self.Value[0].N)

    def MarshalBinary(self) -> bytes:
        meta = wire.metadata_marshal(0, None, False, False, 0, 0, self.IsNTT, False)
        return wire.ciphertext_marshal(np.stack([v.download()[0] for v in self.Value]), meta)


class PublicKeySwitchProtocol:
    """multiparty.NewPublicKeySwitchProtocol(params, noiseFlooding = DiscreteGaussian{Sigma: noiseSigma}): `encryptor` is the party's
    rlwe.Encryptor (its own source); the smudging noise DiscreteGaussian{sqrt(NoiseFreshSK^2 + noiseSigma^2), 6 sigma}
    (keyswitch_pk.go:41-47) is read from `noise_prng`"""

    def __init__(self, encryptor: Encryptor, noise_prng: PRNG, noiseSigma: float, NoiseFreshSK: float):
        self.Encryptor, self.noise_prng = encryptor, noise_prng
        self.Sigma = math.sqrt(float(NoiseFreshSK) ** 2 + float(noiseSigma) ** 2)
        self.Bound = 6 * self.Sigma

    def AllocateShare(self, levelQ: int) -> PublicKeySwitchShare:
        rq = self.Encryptor.evaluator.ringQ.AtLevel(levelQ)
        return PublicKeySwitchShare([rq.NewPoly(), rq.NewPoly()])

    def GenShare(self, sk: SecretKey, pk: PublicKey, ct: Element, shareOut: PublicKeySwitchShare):
        level = min(shareOut.Level(), ct.Value[1].n_limbs - 1)  # :71
        enc = self.Encryptor.WithKey(pk)
        try:
            check(load().he_mp_pcks_gen_share(enc.h, self.noise_prng.h, level, sk.Q.h, ct.Value[1].h, int(ct.IsNTT), int(ct.IsMontgomery), self.Sigma,
                                              self.Bound, shareOut.Value[0].h, shareOut.Value[1].h))
        except Exception as e:
            for src in (self.Encryptor.prng, self.noise_prng):  # a reader's own exception is the cause
                cause, src.error = src.error, None
                if cause is not None:
                    raise e from cause
            raise

    def AggregateShares(self, share1: PublicKeySwitchShare, share2: PublicKeySwitchShare, shareOut: PublicKeySwitchShare):
        if share1.Value[0].n_limbs != share1.Value[1].n_limbs:
            raise ValueError("cannot AggregateShares: the two shares are at different levelQ")
        rq = self.Encryptor.evaluator.ringQ
        for k in range(2):
            check(load().he_add(rq.h, share1.Level(), share1.Value[k].h, share2.Value[k].h, shareOut.Value[k].h))

    def KeySwitch(self, ctIn: Element, combined: PublicKeySwitchShare, opOut: Element):
        level = ctIn.Value[0].n_limbs - 1
        if ctIn is not opOut:
            opOut.IsNTT, opOut.IsMontgomery = ctIn.IsNTT, ctIn.IsMontgomery
        check(load().he_add(self.Encryptor.evaluator.ringQ.h, level, ctIn.Value[0].h, combined.Value[0].h, opOut.Value[0].h))
        check(load().he_poly_copy(opOut.Value[1].h, combined.Value[1].h, level))


__all__ = ["PublicKeySwitchProtocol", "PublicKeySwitchShare", "EvaluationKeyGenProtocol", "GaloisKeyGenProtocol", "EvaluationKeyGenCRP", "EvaluationKeyGenShare", "GaloisKeyGenCRP",
           "GaloisKeyGenShare", "RelinearizationKeyGenProtocol", "RelinearizationKeyGenCRP", "RelinearizationKeyGenShare",
           "PublicKeyGenProtocol", "PublicKeyGenCRP", "PublicKeyGenShare", "KeySwitchProtocol", "KeySwitchCRP", "KeySwitchShare"]
