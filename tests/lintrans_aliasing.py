"""Operand identity at the entry points of include/hering_lintrans.h, as rows of tests/aliasing_table.Row (the table of
include/hering.h stays as it is: these entries live in their own header).  tests/test_gpu_lintrans.py runs every pair, allowed
and rejected, and checks that a rejected call leaves every operand unchanged.

he_lintrans_evaluate (n_lt == 1): P * ct, the copy the naive form keeps for its zero diagonal, the decomposition and every
pre-rotation are taken before the first output word is written, so each output may be each input.  he_lintrans_evaluate_many with
n_lt > 1: transformation k + 1 still reads what transformation k would have overwritten -- no output may be an input.  Whatever
n_lt: two outputs that are one polynomial (of one transformation or of two) and an output that is a diagonal are rejected."""
from tests.aliasing_table import IN, OUT, Q, Row

ROWS = {
    "he_lintrans_evaluate": Row("he_lintrans_evaluate", {"in0": (IN, Q), "in1": (IN, Q), "out0": (OUT, Q), "out1": (OUT, Q)},
                                "lintrans.Evaluator.Evaluate(ctLevel, ctIn, lt, opOut)",
                                {(o, i) for o in ("out0", "out1") for i in ("in0", "in1")},
                                oracle="LinTransEvaluator.EvaluateMany(ct, [lt]) on the pre-call words"),
    "he_lintrans_evaluate_many": Row("he_lintrans_evaluate_many", {"in0": (IN, Q), "in1": (IN, Q), "out0": (OUT, Q), "out1": (OUT, Q)},
                                     "lintrans.Evaluator.EvaluateMany(ctLevel, ctIn, lts, opOut)   (n_lt > 1)", set(),
                                     oracle="LinTransEvaluator.EvaluateMany(ct, lts)", arrays=("out0", "out1")),
}
