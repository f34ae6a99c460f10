"""Operand identity at the entry point of include/hering_polyeval.h that takes polynomials, as a row of tests/aliasing_table.Row
(the table of include/hering.h stays as it is: this entry lives in its own header).  tests/test_gpu_polyeval.py runs every pair
and checks that a rejected call leaves every operand unchanged.

he_polyeval_leaves: every workgroup reads its words of every power before it writes, but another baby step of the same call, or
another limb's workgroup of a component that is also a power, may not have read them yet -- no output may be a power.  Two
outputs that are one polynomial are rejected as everywhere."""
from tests.aliasing_table import IN, OUT, Q, Row

ROWS = {
    "he_polyeval_leaves": Row("he_polyeval_leaves", {"x": (IN, Q), "out": (OUT, Q)},
                              "polynomial.Evaluator.EvaluatePolynomialVectorFromPowerBasis(targetLevel, pol, pb, targetScale)", set(),
                              oracle="Add(res, c_0), MulThenAdd(X[k], c_k, res) for k = deg ... 1 on the pre-call words",
                              arrays=("x", "out")),
    # Evaluate copies its input into X^1 first, but the reference's result is a new ciphertext: no output may be the input
    "he_polyeval_evaluate": Row("he_polyeval_evaluate", {"in0": (IN, Q), "in1": (IN, Q), "out0": (OUT, Q), "out1": (OUT, Q)},
                                "polynomial.Evaluator.Evaluate(ct, p, targetScale)", set(),
                                oracle="polyeval_ref.evaluate_polynomial on the pre-call words"),
    # ... and none may be a component of a power of the basis (borrowed through he_polyeval_basis_power)
    "he_polyeval_evaluate_from_power_basis": Row("he_polyeval_evaluate_from_power_basis", {"out0": (OUT, Q), "out1": (OUT, Q)},
                                                 "polynomial.Evaluator.EvaluateFromPowerBasis(pb, p, targetScale)", set(),
                                                 oracle="polyeval_ref on the basis' words"),
}
