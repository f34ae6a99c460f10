"""Operand identity at the entry points of include/hering_bridge.h, as rows of tests/aliasing_table.Row (the table of
include/hering.h stays as it is: these entries live in their own header).  Every entry has its inputs at one degree and its
outputs at the other, and handles of different degree never coincide: no (output, input) pair is allowed, the two outputs of a
ciphertext entry are rejected, and in0 == in1 is two inputs (accepted)."""
from tests.aliasing_table import IN, OUT, Q, Row

_CT = {"in0": (IN, Q), "in1": (IN, Q), "out0": (OUT, Q), "out1": (OUT, Q)}

ROWS = {
    "he_unfold_conjugate_invariant_to_standard": Row("he_unfold_conjugate_invariant_to_standard",
                                                     {"polyConjugateInvariant": (IN, Q), "polyStandard": (OUT, Q)},
                                                     "Ring.UnfoldConjugateInvariantToStandard(polyConjugateInvariant, polyStandard)",
                                                     oracle="polyStandard := concat(in, reversed(in))"),
    "he_fold_standard_to_conjugate_invariant": Row("he_fold_standard_to_conjugate_invariant",
                                                   {"polyStandard": (IN, Q), "polyConjugateInvariant": (OUT, Q)},
                                                   "Ring.FoldStandardToConjugateInvariant(polyStandard, polyConjugateInvariant)",
                                                   oracle="out[j] := CRed(in[N-1-j] + in[j])"),
    "he_complex_to_real": Row("he_complex_to_real", dict(_CT), "bridge.DomainSwitcher.ComplexToReal(ctIn, opOut)",
                              oracle="Fold(GadgetProduct(in1) + (in0, 0))"),
    "he_real_to_complex": Row("he_real_to_complex", dict(_CT), "bridge.DomainSwitcher.RealToComplex(ctIn, opOut)",
                              oracle="GadgetProduct(Unfold(in1)) + (Unfold(in0), 0)"),
}
