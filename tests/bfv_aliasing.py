"""Operand identity at the entry points of include/hering_bfv.h, as rows of tests/aliasing_table.Row (the table of
include/hering.h stays as it is: these entries live in their own header).  he_bfv_mul_relin consumes its inputs into scratch
before it writes the first output word: every (output, input) pair is an in-place form, two outputs never are.  he_bfv_quantize
writes outQ over cQ; cM lives on the QMul side and is no other operand."""
from tests.aliasing_table import IN, OUT, P, Q, Row, _all_pairs

_MUL = {"a0": (IN, Q), "a1": (IN, Q), "b0": (IN, Q), "b1": (IN, Q), "out0": (OUT, Q), "out1": (OUT, Q), "out2": (OUT, Q)}

ROWS = {
    "he_bfv_mul_relin": Row("he_bfv_mul_relin", dict(_MUL), "bfv.ScaleInvariantEvaluator.MulRelinScaleInvariant(level, op0, op1, rlk, opOut)",
                            _all_pairs(_MUL), oracle="circuits.ScaleInvariantEvaluator.MulRelinScaleInvariant on the pre-call words"),
    "he_bfv_quantize": Row("he_bfv_quantize", {"cQ": (IN, Q), "cM": (IN, P), "outQ": (OUT, Q)},
                           "bfv.ScaleInvariantEvaluator.Quantize(level, c2Q1, c2Q2, opOut)", {("outQ", "cQ")},
                           oracle="circuits.ScaleInvariantEvaluator._quantize on the pre-call words"),
}
