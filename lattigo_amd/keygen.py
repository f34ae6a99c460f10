"""rlwe.KeyGenerator on the device (include/hering_keygen.h; core/rlwe/keygenerator.go), the sparse ternary sampler
(ring/sampler_ternary.go:198-263) and AddPolyTimesGadgetVectorToGadgetCiphertext (core/rlwe/gadgetciphertext.go:172-241).  Every call
is an exact function of the byte stream of the generator's PRNG: the words, the drawing order (an evaluation key: row after row,
the uniform c1 and then the Gaussian e; Galois keys: key after key) and the position of the source afterwards are the
reference's.  The keys returned are rlwe.EvaluationKey objects that the Evaluator's methods take as they are."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

from . import encryptor as _enc
from ._lib import H, check, load
from .encryptor import DefaultXeBound, DefaultXeSigma, DefaultXsP, PublicKey, SecretKey, _h
from .ring import Poly, Ring
from .rlwe import BaseRNSDecompositionVectorSize, EvaluationKey, Evaluator
from .sampling import PRNG


@dataclass
class EvaluationKeyParameters:
    """rlwe.EvaluationKeyParameters (core/rlwe/evaluationkey.go): None = the parameters' default"""
    LevelQ: int | None = None
    LevelP: int | None = None
    BaseTwoDecomposition: int | None = None
    Compressed: bool = False


@dataclass
class GaloisKey:
    """rlwe.GaloisKey: the evaluation key with its Galois element and NthRoot"""
    EvaluationKey: EvaluationKey
    GaloisElement: int
    NthRoot: int


class SparseTernarySampler:
    """ring.NewTernarySampler(prng, baseRing, Ternary{H: H}, montgomery): Read only"""

    def __init__(self, prng: PRNG, baseRing: Ring, H: int, montgomery: bool):
        self.prng, self.baseRing, self.H, self.montgomery = prng, baseRing, int(H), bool(montgomery)

    def AtLevel(self, level: int) -> "SparseTernarySampler":
        return SparseTernarySampler(self.prng, self.baseRing.AtLevel(level), self.H, self.montgomery)

    def Read(self, pol: Poly):
        self.prng.check(load().he_keygen_ternary_sparse_read(self.baseRing.h, self.baseRing.Level(), self.prng.h, self.H, int(self.montgomery), pol.h))

    def ReadNew(self) -> Poly:
        pol = self.baseRing.NewPoly()
        self.Read(pol)
        return pol


def AddPolyTimesGadgetVectorToGadgetCiphertext(pt: Poly, cts):
    """pt times the gadget vector added to component u of cts[u] (one or two keys)"""
    if not 1 <= len(cts) <= 2:
        raise ValueError("cannot AddPolyTimesGadgetVectorToGadgetCiphertext: len(cts) should be <= 2")
    check(load().he_gadget_add_poly(pt.h, cts[0].h, cts[1].h if len(cts) > 1 else 0))


def BaseTwoDecompositionVectorSize(moduliQ, levelQ: int, levelP: int, Base2Decomposition: int):
    """core/rlwe/params.go:523-540, over limbs 0..levelQ"""
    if Base2Decomposition == 0 or levelP > 0:
        return [1] * (levelQ + 1)
    return [(int(round(math.log2(float(q)))) + Base2Decomposition - 1) // Base2Decomposition for q in moduliQ[:levelQ + 1]]


class KeyGenerator(_enc.KeyGenerator):
    """rlwe.NewKeyGenerator(params) over the rings of `evaluator`"""

    def __init__(self, evaluator: Evaluator, prng: PRNG, XsP: float = DefaultXsP, XeSigma: float = DefaultXeSigma, XeBound: float = DefaultXeBound):
        super().__init__(evaluator, prng, XsP, XeSigma, XeBound)
        h = H()
        check(load().he_keygen_create(evaluator.h, prng.h, float(XsP), float(XeSigma), float(XeBound), C.byref(h)))
        self.h = h.value

    def __del__(self):
        try:
            if getattr(self, "h", None):
                load().he_keygen_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # -- secret and public keys
    def _new_sk(self) -> SecretKey:
        rq, rp = self.evaluator.ringQ, self.evaluator.ringP
        return SecretKey(rq.NewPoly(), rp.NewPoly() if rp is not None else None)

    def GenSecretKey(self, sk: SecretKey):
        self.prng.check(load().he_keygen_secret_key(self.h, sk.Q.Level(), -1 if sk.P is None else sk.P.Level(), sk.Q.h, _h(sk.P)))

    def GenSecretKeyNew(self) -> SecretKey:
        sk = self._new_sk()
        self.GenSecretKey(sk)
        return sk

    def GenSecretKeyWithHammingWeight(self, hw: int, sk: SecretKey):
        self.prng.check(load().he_keygen_secret_key_hw(self.h, int(hw), sk.Q.Level(), -1 if sk.P is None else sk.P.Level(), sk.Q.h, _h(sk.P)))

    def GenSecretKeyWithHammingWeightNew(self, hw: int) -> SecretKey:
        sk = self._new_sk()
        self.GenSecretKeyWithHammingWeight(hw, sk)
        return sk

    def GenKeyPairNew(self):
        sk = self.GenSecretKeyNew()
        return sk, self.GenPublicKeyNew(sk)

    # -- evaluation keys
    def _resolve(self, evkParams):
        """ResolveEvaluationKeyParameters (core/rlwe/evaluationkey.go)"""
        rq, rp = self.evaluator.ringQ, self.evaluator.ringP
        p = evkParams or EvaluationKeyParameters()
        if p.Compressed:
            raise NotImplementedError("compressed evaluation keys are not on the device (include/hering_keygen.h)")
        levelQ = rq.MaxLevel() if p.LevelQ is None else p.LevelQ
        levelP = (rp.MaxLevel() if rp is not None else -1) if p.LevelP is None else p.LevelP
        return levelQ, levelP, p.BaseTwoDecomposition or 0

    def NewEvaluationKey(self, evkParams: EvaluationKeyParameters | None = None) -> EvaluationKey:
        """newEvaluationKey: a zeroed key of degree 1 at the resolved levels"""
        levelQ, levelP, pw2 = self._resolve(evkParams)
        beta = BaseRNSDecompositionVectorSize(levelQ, levelP)
        if pw2:
            nj = BaseTwoDecompositionVectorSize(self.evaluator.ringQ.moduli, levelQ, levelP, pw2)
            return EvaluationKey(self.evaluator, None, None, pw2, nj, shape=(sum(nj), levelQ + 1, levelP + 1))
        return EvaluationKey(self.evaluator, None, None, shape=(beta, levelQ + 1, levelP + 1))

    def GenEvaluationKey(self, skInput: SecretKey, skOutput: SecretKey, evk: EvaluationKey):
        """GenEvaluationKey (:261-285): the two keys may live in rings of a smaller degree and at other levels; only their Q parts
        are read (skOutput.P is rebuilt from limb 0 of skOutput.Q, as the reference does)"""
        self.prng.check(load().he_keygen_evaluation_key_sk(self.h, skInput.Q.h, skOutput.Q.h, evk.h))

    def genEvaluationKey(self, skIn: Poly, skOut: SecretKey, evk: EvaluationKey):
        """genEvaluationKey (:287-330) on operands of the key's own ring and levels: the fused entry"""
        self.prng.check(load().he_keygen_evaluation_key(self.h, skIn.h, skOut.Q.h, _h(skOut.P), evk.h))

    def GenEvaluationKeyNew(self, skInput: SecretKey, skOutput: SecretKey, evkParams: EvaluationKeyParameters | None = None) -> EvaluationKey:
        evk = self.NewEvaluationKey(evkParams)
        self.GenEvaluationKey(skInput, skOutput, evk)
        return evk

    def GenEvaluationKeysForRingSwapNew(self, skStd: SecretKey, skConjugateInvariant: SecretKey, evkParams: EvaluationKeyParameters | None = None):
        """(:211-233) over he_unfold_conjugate_invariant_to_standard: (stdToci, ciToStd).  skCIMappedToStandard.P is not built here:
        GenEvaluationKey rebuilds the P part of its output key itself"""
        rq = self.evaluator.ringQ
        levelQ = min(skStd.Q.Level(), skConjugateInvariant.Q.Level())
        mapped = SecretKey(Poly(rq, levelQ + 1), None)
        check(load().he_unfold_conjugate_invariant_to_standard(levelQ, skConjugateInvariant.Q.h, mapped.Q.h))
        return self.GenEvaluationKeyNew(skStd, mapped, evkParams), self.GenEvaluationKeyNew(mapped, skStd, evkParams)

    def GenRelinearizationKey(self, sk: SecretKey, rlk: EvaluationKey):
        self.prng.check(load().he_keygen_relinearization_key(self.h, sk.Q.h, _h(sk.P), rlk.h))

    def GenRelinearizationKeyNew(self, sk: SecretKey, evkParams: EvaluationKeyParameters | None = None) -> EvaluationKey:
        rlk = self.NewEvaluationKey(evkParams)
        self.GenRelinearizationKey(sk, rlk)
        return rlk

    def GenGaloisKey(self, galEl: int, sk: SecretKey, gk: GaloisKey | EvaluationKey):
        evk = gk.EvaluationKey if isinstance(gk, GaloisKey) else gk
        self.prng.check(load().he_keygen_galois_key(self.h, int(galEl), sk.Q.h, _h(sk.P), evk.h))
        if isinstance(gk, GaloisKey):
            gk.GaloisElement, gk.NthRoot = int(galEl), self.evaluator.ringQ.NthRoot()

    def GenGaloisKeyNew(self, galEl: int, sk: SecretKey, evkParams: EvaluationKeyParameters | None = None) -> GaloisKey:
        gk = GaloisKey(self.NewEvaluationKey(evkParams), int(galEl), self.evaluator.ringQ.NthRoot())
        self.GenGaloisKey(galEl, sk, gk)
        return gk

    def GenGaloisKeys(self, galEls, sk: SecretKey, gks):
        """gks[i] None: a new key at the default levels, as the reference"""
        if len(galEls) != len(gks):
            raise ValueError("galEls and gks must have the same length")
        for i, g in enumerate(galEls):
            if gks[i] is None:
                gks[i] = GaloisKey(self.NewEvaluationKey(), int(g), self.evaluator.ringQ.NthRoot())
        n = len(galEls)
        els = (C.c_uint64 * max(n, 1))(*[int(g) for g in galEls])
        hs = (C.c_uint64 * max(n, 1))(*[(k.EvaluationKey if isinstance(k, GaloisKey) else k).h for k in gks])
        self.prng.check(load().he_keygen_galois_keys(self.h, n, els, sk.Q.h, _h(sk.P), hs))
        for g, k in zip(galEls, gks):
            if isinstance(k, GaloisKey):
                k.GaloisElement, k.NthRoot = int(g), self.evaluator.ringQ.NthRoot()

    def GenGaloisKeysNew(self, galEls, sk: SecretKey, evkParams: EvaluationKeyParameters | None = None):
        gks = [GaloisKey(self.NewEvaluationKey(evkParams), int(g), self.evaluator.ringQ.NthRoot()) for g in galEls]
        self.GenGaloisKeys(galEls, sk, gks)
        return gks


__all__ = ["KeyGenerator", "EvaluationKeyParameters", "GaloisKey", "SparseTernarySampler", "AddPolyTimesGadgetVectorToGadgetCiphertext",
           "BaseTwoDecompositionVectorSize", "SecretKey", "PublicKey"]
