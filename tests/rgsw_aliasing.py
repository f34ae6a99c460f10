"""Operand identity at the product entries of include/hering_rgsw.h, as rows of tests/aliasing_table.Row (the table of
include/hering.h stays as it is: these entries live in their own header).  out0 == in0 and out1 == in1 are the reference's
op0 == opOut; in0 == in1 reads one polynomial twice; every other pair, out0 == out1 included, is refused."""
from tests.aliasing_table import IN, OUT, Q, Row

_PARAMS = {"in0": (IN, Q), "in1": (IN, Q), "out0": (OUT, Q), "out1": (OUT, Q)}
_INPLACE = {("out0", "in0"), ("out1", "in1")}

ROWS = {
    "he_rgsw_external_product": Row("he_rgsw_external_product", dict(_PARAMS),
                                    "rgsw.Evaluator.ExternalProduct(op0, op1, opOut)", set(_INPLACE),
                                    oracle="tests.rgsw_ref.external_product on the pre-call words"),
    "he_rgsw_external_product_select": Row("he_rgsw_external_product_select", dict(_PARAMS),
                                           "rgsw.Evaluator.ExternalProductSelect(op0, keys, sel, opOut)", set(_INPLACE),
                                           oracle="tests.rgsw_ref.external_product per entry with key sel[b]; sel[b] == -1: the entry itself"),
}
