"""Operand identity at the two polynomial entries of include/hering_blindrot.h, as rows of tests/aliasing_table.Row (as
tests/rgsw_aliasing.py: these entries live in their own header).  he_automorphism_ct_select: out0 == in0 and out1 == in1 give the
words of the out-of-place call, in0 == in1 reads one polynomial twice, every other pair is refused.  he_blind_rotate_core works in
place on (acc0, acc1): two accumulators that start from their own words, which must be distinct."""
from tests.aliasing_table import ACC, IN, OUT, Q, Row

ROWS = {
    "he_automorphism_ct_select": Row("he_automorphism_ct_select", {"in0": (IN, Q), "in1": (IN, Q), "out0": (OUT, Q), "out1": (OUT, Q)},
                                     "blindrot.AutomorphismSelect(evaluator, ctIn, keys, sel, opOut)", {("out0", "in0"), ("out1", "in1")},
                                     oracle="oracle.Evaluator.Automorphism per entry with key sel[b] and its Galois element; sel[b] == -1: "
                                            "the entry itself"),
    "he_blind_rotate_core": Row("he_blind_rotate_core", {"acc0": (ACC, Q), "acc1": (ACC, Q)},
                                "blindrot.Evaluator.BlindRotateCore(a, acc, BRK)", set(),
                                oracle="tests.blindrot_ref.blind_rotate_core on the pre-call words"),
}
