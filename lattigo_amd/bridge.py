"""ckks.DomainSwitcher (schemes/ckks/bridge.go): the bridge between standard CKKS ciphertexts in Z[X]/(X^N+1) (complex slots) and
conjugate-invariant ones in Z[X+X^-1]/(X^N+1), held in compressed form with N/2 words per limb (real slots), on the device
(include/hering_bridge.h)."""
from __future__ import annotations

from ._lib import HeringError, check, load


class DomainSwitcher:
    """ckks.DomainSwitcher (bridge.go:13-47).  `evaluator`: the rlwe Evaluator of the standard ring of degree N (bridge.go takes
    it per call; the keys are bound to one evaluator here, so it is given once); `stdToci` / `ciToStd`: the two keys of
    KeyGenerator.GenEvaluationKeysForRingSwap as device EvaluationKeys of that evaluator, or None.

    Ciphertexts are pairs of Poly (c0, c1) without metadata, NTT domain, degree 1: after ComplexToReal the caller doubles the
    scale it keeps for the ciphertext (bridge.go:93: opOut.Scale = ctIn.Scale * 2); RealToComplex leaves it as it is."""

    def __init__(self, evaluator, stdToci=None, ciToStd=None):
        self.evaluator = evaluator
        self.stdToci = stdToci
        self.ciToStd = ciToStd

    def ComplexToReal(self, ctIn, opOut):
        """bridge.go:57-95: ctIn of degree N -> opOut of degree N/2 at level min(ctIn.Level(), opOut.Level()):
        opOut_k = Fold(GadgetProduct(ctIn[1], stdToci)_k + (k == 0) ctIn[0]).  The scale of the result is twice ctIn's."""
        level = min(ctIn[0].Level(), opOut[0].Level())
        if self.stdToci is None:
            raise HeringError(-1, "cannot ComplexToReal: no realToComplexEvk provided to this DomainSwitcher")
        check(load().he_complex_to_real(self.evaluator.h, level, ctIn[0].h, ctIn[1].h, self.stdToci.h, opOut[0].h, opOut[1].h))

    def RealToComplex(self, ctIn, opOut):
        """bridge.go:104-144: ctIn of degree N/2 -> opOut of degree N at level min(ctIn.Level(), opOut.Level()):
        (u0, u1) = Unfold(ctIn), opOut = (u0 + GadgetProduct(u1, ciToStd)_0, GadgetProduct(u1, ciToStd)_1)."""
        level = min(ctIn[0].Level(), opOut[0].Level())
        if self.ciToStd is None:
            raise HeringError(-1, "cannot RealToComplex: no realToComplexEvk provided to this DomainSwitcher")
        check(load().he_real_to_complex(self.evaluator.h, level, ctIn[0].h, ctIn[1].h, self.ciToStd.h, opOut[0].h, opOut[1].h))
