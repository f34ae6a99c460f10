"""Operand identity at the entry points of include/hering_ckks_evaluator.h, as rows of tests/aliasing_table.Row (the table of
include/hering.h stays as it is: these entries live in their own header).  tests/test_gpu_ckks_evaluator.py runs every allowed
form against the restatement on the pre-call words and every refused one, checking that it leaves every operand unchanged.

he_ckks_add, he_ckks_scalar, he_ckks_mul_pt: one thread owns a coefficient pair of every component and reads all of its input
words before it writes, so any output may be any input, crossed components included.  he_ckks_mul_relin_then_add: the
reference refuses an output that is an input (schemes/ckks/evaluator.go:918, :1064), and the key switch reads its operands from
other workgroups.  Two outputs that are one polynomial are refused everywhere."""
from tests.aliasing_table import ACC, IN, OUT, Q, Row

ROWS = {
    "he_ckks_add": Row("he_ckks_add", {"op0": (IN, Q), "op1": (IN, Q), "out": (OUT, Q)},
                       "lattigo_amd.ckks.ct_add(ring, op0, op1, out, sub=, scaled=, ratio=)", {("out", "op0"), ("out", "op1")},
                       oracle="tests/ckks_evaluator_ref.ckks_add on the pre-call words", arrays=("op0", "op1", "out")),
    "he_ckks_scalar": Row("he_ckks_scalar", {"op0": (IN, Q), "out": (ACC, Q)}, "lattigo_amd.ckks.ct_scalar(ring, op, op0, s0, s1, out, pre=)",
                          {("out", "op0")}, oracle="tests/ckks_evaluator_ref.ckks_scalar on the pre-call words", arrays=("op0", "out")),
    "he_ckks_mul_pt": Row("he_ckks_mul_pt", {"ct": (IN, Q), "pt": (IN, Q), "out": (ACC, Q)},
                          "lattigo_amd.ckks.ct_mul_pt(ring, ct, pt, out, then_add=, pre=)", {("out", "ct"), ("out", "pt")},
                          oracle="tests/ckks_evaluator_ref.ckks_mul_pt on the pre-call words", arrays=("ct", "out")),
    "he_ckks_mul_relin_then_add": Row("he_ckks_mul_relin_then_add",
                                      {"a0": (IN, Q), "a1": (IN, Q), "b0": (IN, Q), "b1": (IN, Q), "out0": (ACC, Q), "out1": (ACC, Q), "out2": (ACC, Q)},
                                      "lattigo_amd.ckks.ct_mul_relin_then_add(evaluator, level, a, b, rlk, out, pre=)", set(),
                                      oracle="tests/ckks_evaluator_ref.ckks_mul_relin_then_add on the pre-call words"),
}
