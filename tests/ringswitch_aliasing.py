"""Operand identity at the two-polynomial entry points of include/hering_ringswitch.h, as rows of tests/aliasing_table.Row (the
table of include/hering.h stays as it is: these entries live in their own header).  Handles of different degree never coincide,
so the allowed pairs are the equal-degree forms: the maps are copies there (x onto x: a no-op), and ApplyEvaluationKey takes any
output on any input, as he_relinearize."""
from tests.aliasing_table import IN, OUT, Q, Row

ROWS = {
    "he_map_small_to_large_ntt": Row("he_map_small_to_large_ntt", {"polSmall": (IN, Q), "polLarge": (OUT, Q)},
                                     "ring.MapSmallDimensionToLargerDimensionNTT(polSmall, polLarge)", {("polLarge", "polSmall")},
                                     oracle="polLarge := repeat(polSmall, gap)"),
    "he_switch_ring_degree_ntt": Row("he_switch_ring_degree_ntt", {"in": (IN, Q), "out": (OUT, Q)},
                                     "rlwe.SwitchCiphertextRingDegreeNTT(ctIn, ringQLargeDim, opOut)", {("out", "in")},
                                     oracle="NTT_n(INTT_N(in)[::gap]) / repeat(in, gap)"),
    "he_switch_ring_degree": Row("he_switch_ring_degree", {"in": (IN, Q), "out": (OUT, Q)},
                                 "rlwe.SwitchCiphertextRingDegree(ctIn, opOut)", {("out", "in")},
                                 oracle="out[::gap] := in / out := in[::gap]"),
    "he_apply_evaluation_key": Row("he_apply_evaluation_key", {"in0": (IN, Q), "in1": (IN, Q), "out0": (OUT, Q), "out1": (OUT, Q)},
                                   "rlwe.Evaluator.ApplyEvaluationKey(level, ctIn, evk, opOut)",
                                   {(o, i) for o in ("out0", "out1") for i in ("in0", "in1")},
                                   oracle="GadgetProduct(in1) + (in0, 0), with the degree maps before / after"),
}
