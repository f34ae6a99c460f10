"""BFV: the scale-invariant multiplication of the reference's bgv.Evaluator with ScaleInvariant = true
(schemes/bgv/evaluator.go:898-1071: tensorScaleInvariant / modUpAndNTT / tensorLowDeg / quantize, precomputation
newEvaluatorPrecomp :38-70) as ONE native call on the device (include/hering_bfv.h)."""
from __future__ import annotations

import ctypes as C

from ._lib import H, check, load
from .ring import Poly, Ring
from .rlwe import EvaluationKey, Evaluator


class ScaleInvariantEvaluator:
    """bgv.Evaluator with ScaleInvariant = true, restricted to ct x ct MulRelinScaleInvariant.  `evaluator`: the rlwe Evaluator of
    the parameters (RingQ, RingP); `ringQMul`: Parameters.RingQMul() (schemes/bgv/params.go:98-109); `t`: the plaintext modulus.

    Ciphertexts are lists of Poly [c0, c1(, c2)] without metadata, NTT domain; the scale of the result is the caller's to record
    (MulScaleInvariant(params, a, b, level), evaluator.go:983).  The signature is that of tests/drivers/bgv.py, the same
    multiplication driven operator by operator."""

    def __init__(self, evaluator: Evaluator, ringQMul: Ring, t: int):
        self.eval, self.t = evaluator, int(t)
        self.ringQ, self.ringQMul = evaluator.ringQ, ringQMul
        h = H()
        check(load().he_bfv_evaluator_create(evaluator.h, ringQMul.h, self.t, C.byref(h)))
        self.h = h.value
        self.levelQMul = []  # evaluator.go:43-48
        for level in range(self.ringQ.MaxLevel() + 1):
            lm = C.c_int()
            check(load().he_bfv_level_qmul(self.h, level, C.byref(lm)))
            self.levelQMul.append(int(lm.value))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                load().he_bfv_evaluator_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def MulRelinScaleInvariant(self, level, op0, op1, rlk: EvaluationKey | None, opOut):
        """tensorScaleInvariant (:898): op0, op1 = [c0, c1] NTT at `level` (op1 is op0, or the same two polynomials: the squaring
        branch); opOut = [c0, c1] with a relinearisation key, [c0, c1, c2] without.  Any polynomial of opOut may be one of the
        inputs."""
        check(load().he_bfv_mul_relin(self.h, level, op0[0].h, op0[1].h, op1[0].h, op1[1].h, rlk.h if rlk is not None else 0,
                                      opOut[0].h, opOut[1].h, opOut[2].h if rlk is None else 0))

    def Quantize(self, level, c2Q1: Poly, c2Q2: Poly, opOut: Poly | None = None):
        """quantize (:1050): c2Q1 on the limbs 0..level of Q and c2Q2 on the limbs 0..levelQMul[level] of QMul, NTT domain ->
        opOut (default: c2Q1, as the reference and the driver's _quantize) = NTT(t * round(INTT(c2Q1 | c2Q2) / Q)), canonical."""
        check(load().he_bfv_quantize(self.h, level, c2Q1.h, c2Q2.h, (c2Q1 if opOut is None else opOut).h))
