"""Operand identity at every entry point of include/hering.h that takes two or more polynomial handles.

One row per entry point: its polynomial parameters in header order with their roles, the Python wrapper that reaches it, how the
reference result of an accepted aliased call is formed, and the (output, input) pairs the entry may be called with in place.  The
rule (hering.h, Conventions): inputs may alias inputs; an output may alias an input of the same side only where the row allows it;
two outputs, and a Q-side and a P-side operand of which one is written, never.  Everything else fails with HE_EINVAL before the
call files anything.

tests/test_aliasing_table.py holds this table against the header; tests/test_gpu_aliasing.py runs every pattern on the device.
This is a plain helper module (not a conftest)."""
from __future__ import annotations

import itertools
from dataclasses import dataclass, field

# roles: "in" read only, "out" overwritten, "acc" an output that starts from its own pre-call words (...ThenAdd, accumulate)
IN, OUT, ACC = "in", "out", "acc"
Q, P = "Q", "P"

# the oracle's out-of-place result of an accepted aliased call is computed on the pre-call words of every operand (so an output
# that is also an input, addend or accumulator starts from its own pre-call words); `oracle` names the oracle/oracle.py calls,
# tests/test_gpu_aliasing.py::_oracle evaluates them
OUT_OF_PLACE = "oracle Ring / BasisExtender / Evaluator method of the same name on the pre-call words"


@dataclass
class Row:
    name: str                      # C entry point
    params: dict                   # polynomial parameter -> (role, side), header order (arrays: one entry per array)
    wrapper: str                   # Python wrapper call (lattigo_amd.ring / .rlwe / .ringqp), or the raw ABI call
    allowed: set = field(default_factory=set)  # {(output, input)} pairs that may be one handle
    oracle: str = OUT_OF_PLACE
    arrays: tuple = ()             # parameters that are handle arrays (const he_handle *)

    def written(self, p):
        return self.params[p][0] in (OUT, ACC)

    def side(self, p):
        return self.params[p][1]

    def verdict(self, a, b):
        """'accept' or 'reject' for parameters a and b being one handle."""
        if not self.written(a) and not self.written(b):
            return "accept"
        if self.written(a) and self.written(b):
            return "reject"
        if self.side(a) != self.side(b):
            return "reject"
        o, i = (a, b) if self.written(a) else (b, a)
        return "accept" if (o, i) in self.allowed else "reject"


def _all_pairs(params):
    """every (output, input) pair of one side: the coefficient-wise operations, computed in place by the reference"""
    outs = [p for p, (r, _) in params.items() if r != IN]
    ins = [p for p, (r, _) in params.items() if r == IN]
    return {(o, i) for o in outs for i in ins if params[o][1] == params[i][1]}


ROWS: dict[str, Row] = {}


def _row(name, params, wrapper, allowed=None, all_inplace=False, **kw):
    params = {k: tuple(v.split(":")) for k, v in params.items()}
    ROWS[name] = Row(name, params, wrapper, _all_pairs(params) if all_inplace else set(allowed or ()), **kw)


# ---- polynomials
_row("he_poly_copy", {"dst": "out:Q", "src": "in:Q"}, "Poly.CopyLvl(level, src)", {("dst", "src")},
     oracle="dst := src (one handle: nothing to copy)")
# overlapping entry ranges of one handle are rejected; disjoint ranges of one handle are distinct operands (the GPU test's own case)
_row("he_poly_copy_batch", {"dst": "out:Q", "src": "in:Q"}, "Poly.CopyBatch(level, dst_b0, src, src_b0, nb)",
     oracle="entries [dst_b0, dst_b0 + nb) := entries [src_b0, src_b0 + nb)")

# ---- NTT and the coefficient-wise operations (ring/operations.go): every output may be every input
for _n, _w in (("he_ntt", "NTT"), ("he_ntt_lazy", "NTTLazy"), ("he_intt", "INTT"), ("he_intt_lazy", "INTTLazy")):
    _row(_n, {"p1": "in:Q", "p2": "out:Q"}, f"Ring.{_w}(p1, p2)", all_inplace=True)
_row("he_binop", {"p1": "in:Q", "p2": "in:Q", "p3": "acc:Q"}, "Ring.binop(name, p1, p2, p3)", all_inplace=True)
_row("he_unop", {"p1": "in:Q", "p2": "out:Q"}, "Ring.unop(name, p1, p2)", all_inplace=True)
_row("he_scalarop", {"p1": "in:Q", "p2": "acc:Q"}, "Ring.scalarop(name, p1, scalar, p2)", all_inplace=True)
_row("he_mul_rns_scalar_montgomery", {"p1": "in:Q", "p2": "out:Q"}, "Ring.MulRNSScalarMontgomery(p1, scalar, p2)", all_inplace=True)
for _n, _w, _r in (("he_add_scalar_bigint", "AddScalarBigint", "out"), ("he_sub_scalar_bigint", "SubScalarBigint", "out"),
                   ("he_mul_scalar_bigint", "MulScalarBigint", "out"), ("he_mul_scalar_bigint_then_add", "MulScalarBigintThenAdd", "acc")):
    _row(_n, {"p1": "in:Q", "p2": f"{_r}:Q"}, f"Ring.{_w}(p1, scalar, p2)", all_inplace=True)
_row("he_double_rns_scalarop", {"p1": "in:Q", "p2": "acc:Q"}, "Ring.MulDoubleRNSScalarThenAdd(p1, s0, s1, p2) (and Add / Sub / Mul)",
     all_inplace=True)
_row("he_shift", {"p1": "in:Q", "p2": "out:Q"}, "Ring.Shift(p1, k, p2)", all_inplace=True)
_row("he_mult_by_monomial", {"p1": "in:Q", "p2": "out:Q"}, "Ring.MultByMonomial(p1, k, p2)", all_inplace=True)
# p2 == vector is not in place: output limb 0 is the vector the other limbs still read (the reference's result differs too)
_row("he_mul_by_vector_montgomery", {"p1": "in:Q", "vector": "in:Q", "p2": "acc:Q"},
     "Ring.MulByVectorMontgomery[ThenAddLazy](p1, vector, p2)", {("p2", "p1")})
for _n, _r in (("he_add", "out"), ("he_sub", "out"), ("he_mul_coeffs_montgomery", "out"), ("he_mul_coeffs_montgomery_then_add", "acc"),
               ("he_mul_coeffs_montgomery_lazy", "out"), ("he_mul_coeffs_montgomery_lazy_then_add_lazy", "acc")):
    _row(_n, {"p1": "in:Q", "p2": "in:Q", "p3": f"{_r}:Q"}, f"ABI {_n}(ring, level, p1, p2, p3)", all_inplace=True)
for _n in ("he_neg", "he_reduce", "he_mform", "he_imform"):
    _row(_n, {"p1": "in:Q", "p2": "out:Q"}, f"ABI {_n}(ring, level, p1, p2)", all_inplace=True)

# ---- rescale: each of the eight variants in place
for _n, _w in (("he_div_round_by_last_modulus_ntt", "DivRoundByLastModulusNTT"), ("he_div_round_by_last_modulus", "DivRoundByLastModulus"),
               ("he_div_floor_by_last_modulus_ntt", "DivFloorByLastModulusNTT"), ("he_div_floor_by_last_modulus", "DivFloorByLastModulus"),
               ("he_div_round_by_last_modulus_many_ntt", "DivRoundByLastModulusManyNTT"),
               ("he_div_round_by_last_modulus_many", "DivRoundByLastModulusMany"),
               ("he_div_floor_by_last_modulus_many_ntt", "DivFloorByLastModulusManyNTT"),
               ("he_div_floor_by_last_modulus_many", "DivFloorByLastModulusMany")):
    _row(_n, {"p0": "in:Q", "p1": "out:Q"}, f"Ring.{_w}([nb, ] p0, p1)", all_inplace=True)
# he_rescale_polys takes arrays: the enumerator spells entry i of array p0 as "p0[i]" (RESCALE_N pairs); a pair may be in place, an
# output that is an operand of another pair may not
RESCALE_N = 2
ROWS["he_rescale_polys"] = Row("he_rescale_polys", {"p0": (IN, Q), "p1": (OUT, Q)}, "Evaluator.Rescale(level, nb, op0, opOut)",
                               {("p1", "p0")}, arrays=("p0", "p1"))

# ---- ring automorphisms: never in place (ring/automorphism.go:37)
_row("he_automorphism_ntt_with_index", {"pin": "in:Q", "pout": "out:Q"}, "Ring.AutomorphismNTTWithIndex(pin, index, pout)")
_row("he_automorphism_ntt_with_index_then_add_lazy", {"pin": "in:Q", "pout": "acc:Q"},
     "Ring.AutomorphismNTTWithIndexThenAddLazy(pin, index, pout)")
_row("he_automorphism", {"pin": "in:Q", "pout": "out:Q"}, "Ring.Automorphism(pin, gal, pout)")

# ---- basis extension
_row("he_modup_q_to_p", {"polQ": "in:Q", "polP": "out:P"}, "BasisExtender.ModUpQtoP(levelQ, levelP, polQ, polP)")
_row("he_modup_p_to_q", {"polP": "in:P", "polQ": "out:Q"}, "BasisExtender.ModUpPtoQ(levelP, levelQ, polP, polQ)")
_row("he_moddown_qp_to_q", {"p1Q": "in:Q", "p1P": "in:P", "p2Q": "out:Q"}, "BasisExtender.ModDownQPtoQ(levelQ, levelP, p1Q, p1P, p2Q)",
     {("p2Q", "p1Q")})
_row("he_moddown_qp_to_q_ntt", {"p1Q": "in:Q", "p1P": "in:P", "p2Q": "out:Q"},
     "BasisExtender.ModDownQPtoQNTT(levelQ, levelP, p1Q, p1P, p2Q)", {("p2Q", "p1Q")})
_row("he_moddown_qp_to_p", {"p1Q": "in:Q", "p1P": "in:P", "p2P": "out:P"}, "BasisExtender.ModDownQPtoP(levelQ, levelP, p1Q, p1P, p2P)",
     {("p2P", "p1P")})

# ---- rlwe.Evaluator
_row("he_decompose_and_split", {"p0Q": "in:Q", "p1Q": "out:Q", "p1P": "out:P"},
     "Evaluator.DecomposeAndSplit(levelQ, levelP, nbPi, digit, p0Q, p1Q, p1P)")
_QP4 = {"c0Q": "out:Q", "c0P": "out:P", "c1Q": "out:Q", "c1P": "out:P"}
_row("he_gadget_product_lazy", {"cx": "in:Q", **_QP4}, "Evaluator.GadgetProductLazy(levelQ, cx, evk, ctQP)")
_row("he_gadget_product_hoisted_lazy", dict(_QP4), "Evaluator.GadgetProductHoistedLazy(levelQ, decomp, evk, ctQP)")
_row("he_gadget_product_hoisted_lazy_digits", dict(_QP4),
     "Evaluator.GadgetProductHoistedLazyDigits(levelQ, decomp, evk, digit_begin, digit_end, ctQP)")
# ModDown runs component by component in the reference: out_k may be c_kQ
_row("he_moddown", {"c0Q": "in:Q", "c0P": "in:P", "c1Q": "in:Q", "c1P": "in:P", "out0": "out:Q", "out1": "out:Q"},
     "Evaluator.ModDown(levelQ, levelP, ctQP, ct)", {("out0", "c0Q"), ("out1", "c1Q")})
_row("he_eval_moddown_qp_to_q_ntt", {"p1Q": "in:Q", "p1P": "in:P", "p2Q": "out:Q"},
     "Evaluator.ModDownQPtoQNTT(levelQ, levelP, p1Q, p1P, p2Q)", {("p2Q", "p1Q")})
_row("he_gadget_product", {"cx": "in:Q", "out0": "out:Q", "out1": "out:Q"}, "Evaluator.GadgetProduct(levelQ, cx, evk, ct)",
     {("out0", "cx"), ("out1", "cx")})
_row("he_gadget_product_hoisted", {"out0": "out:Q", "out1": "out:Q"}, "Evaluator.GadgetProductHoisted(levelQ, decomp, evk, ct)")
_row("he_relinearize", {"in0": "in:Q", "in1": "in:Q", "in2": "in:Q", "out0": "out:Q", "out1": "out:Q"},
     "Evaluator.Relinearize(level, ctIn, rlk, opOut)", all_inplace=True)
_row("he_automorphism_ct", {"in0": "in:Q", "in1": "in:Q", "out0": "out:Q", "out1": "out:Q"},
     "Evaluator.Automorphism(level, ctIn, galEl, gk, opOut)", all_inplace=True)
_row("he_automorphism_hoisted", {"in0": "in:Q", "out0": "out:Q", "out1": "out:Q"},
     "Evaluator.AutomorphismHoisted(level, ctIn, decomp, galEl, gk, opOut)", all_inplace=True)
_row("he_automorphism_hoisted_lazy", {"in0": "in:Q", **_QP4}, "Evaluator.AutomorphismHoistedLazy(levelQ, ctIn, decomp, galEl, gk, ctQP)",
     {("c0Q", "in0"), ("c1Q", "in0")})
for _n, _w in (("he_ckks_mul_relin", "CKKSMulRelin(level, op0, op1, rlk, opOut)"), ("he_bgv_mul_relin", "BGVMulRelin(level, t, op0, op1, rlk, opOut)")):
    _row(_n, {"a0": "in:Q", "a1": "in:Q", "b0": "in:Q", "b1": "in:Q", "out0": "out:Q", "out1": "out:Q", "out2": "out:Q"},
         f"Evaluator.{_w}", all_inplace=True)
_row("he_centered_lift", {"src": "in:Q", "dstQ": "out:Q", "dstP": "out:P"},
     "RingQP.ExtendBasisSmallNormAndCenter / ABI he_centered_lift(eval, strict, src, first_q, levelQ, dstQ, levelP, dstP)",
     {("dstQ", "src")})
_row("he_decomp_fill", {"srcQ": "in:Q", "srcP": "in:P"}, "ABI he_decomp_fill(decomp, levelQ, levelP, srcQ, srcP)")
# the lintrans inner sum: arrays of LINTRANS_N terms; the outputs alias nothing
LINTRANS_N = 2
ROWS["he_lintrans_mul_sum"] = Row(
    "he_lintrans_mul_sum",
    {"ptQ": (IN, Q), "ptP": (IN, P), "ct0Q": (IN, Q), "ct0P": (IN, P), "ct1Q": (IN, Q), "ct1P": (IN, P),
     "out0Q": (ACC, Q), "out0P": (ACC, P), "out1Q": (ACC, Q), "out1P": (ACC, P)},
    "ABI he_lintrans_mul_sum(eval, levelQ, levelP, n, ptQ, ptP, ct0Q, ct0P, ct1Q, ct1P, index, accumulate, out0Q, out0P, out1Q, out1P)",
    arrays=("ptQ", "ptP", "ct0Q", "ct0P", "ct1Q", "ct1P"))
_row("he_lintrans_giant_step", {"cx": "in:Q", "addQ": "in:Q", "addP": "in:P", "c0Q": "acc:Q", "c0P": "acc:P", "c1Q": "acc:Q", "c1P": "acc:P"},
     "Evaluator.LinTransGiantStep(levelQ, cx, gk, galEl, addQP, outQP, accumulate)")


# ---------------------------------------------------------------------------------------------------------------------------
def operands(row: Row) -> list[str]:
    """the row's operands as the GPU test allocates them: array parameters expanded to their entries ("p0[1]")"""
    n = RESCALE_N if row.name == "he_rescale_polys" else LINTRANS_N
    out = []
    for p in row.params:
        out += [f"{p}[{i}]" for i in range(n)] if p in row.arrays else [p]
    return out


def base(op: str) -> str:
    return op.split("[")[0]


def verdict(row: Row, group) -> str:
    """'accept' or 'reject' for one handle passed as every operand of `group`"""
    group = list(group)
    if row.name == "he_rescale_polys":  # a pair may be in place; an output shared with another pair may not
        outs = [o for o in group if base(o) == "p1"]
        if len(outs) > 1 or (outs and any(base(o) == "p0" and o[2:] != outs[0][2:] for o in group)):
            return "reject"
    for a, b in itertools.combinations(group, 2):
        if row.verdict(base(a), base(b)) == "reject":
            return "reject"
    return "accept"


# the triple patterns real callers use
TRIPLES = {
    "he_binop": [[("p1", "p2", "p3")]],                                      # binop(x, x, x)
    "he_add": [[("p1", "p2", "p3")]], "he_mul_coeffs_montgomery": [[("p1", "p2", "p3")]],
    "he_ckks_mul_relin": [[("a0", "b0", "out0"), ("a1", "b1", "out1")],     # MulRelin(res, res, res)
                          [("b1", "out0"), ("a0", "out1")]],                 # crossed outputs (test_gpu_headline.py)
    "he_bgv_mul_relin": [[("a0", "b0", "out0"), ("a1", "b1", "out1")], [("b1", "out0"), ("a0", "out1")]],
    "he_relinearize": [[("in0", "out0"), ("in1", "out1")], [("in1", "out0"), ("in0", "out1")]],
    "he_automorphism_ct": [[("in0", "out0"), ("in1", "out1")], [("in1", "out0"), ("in0", "out1")]],  # Rotate(ct, k, ct)
}


def patterns(row: Row):
    """Every pairwise aliasing pattern of the row's operands, then its triple / multi-group patterns: lists of groups, each group
    the operands that are one handle.  A Q-side and a P-side operand share a Q-ring polynomial of max(levelQ, levelP) + 1 limbs."""
    ops = operands(row)
    for a, b in itertools.combinations(ops, 2):
        yield [(a, b)]
    for groups in TRIPLES.get(row.name, []):
        yield [tuple(g) for g in groups]


def pattern_verdict(row: Row, groups) -> str:
    return "reject" if any(verdict(row, g) == "reject" for g in groups) else "accept"


def pattern_id(groups) -> str:
    return "+".join("=".join(g) for g in groups)


# how the oracle's out-of-place result is formed, per row (oracle/oracle.py; O = the oracle module, oQ / oP its rings)
_ORACLE = {
    "he_add": "oQ.binop('Add')", "he_sub": "oQ.binop('Sub')", "he_mul_coeffs_montgomery": "oQ.binop('MulCoeffsMontgomery')",
    "he_mul_coeffs_montgomery_then_add": "oQ.binop('MulCoeffsMontgomeryThenAdd', p1, p2, p3)",
    "he_mul_coeffs_montgomery_lazy": "oQ.binop('MulCoeffsMontgomeryLazy')",
    "he_mul_coeffs_montgomery_lazy_then_add_lazy": "oQ.binop('MulCoeffsMontgomeryLazyThenAddLazy', p1, p2, p3)",
    "he_neg": "oQ.unop('Neg')", "he_reduce": "oQ.unop('Reduce')", "he_mform": "oQ.unop('MForm')", "he_imform": "oQ.unop('IMForm')",
    "he_poly_copy": "dst[:L] := src[:L]", "he_poly_copy_batch": "dst entries := src entries",
    "he_binop": "oQ.binop(op, p1, p2, p3)", "he_unop": "oQ.unop(op, p1)", "he_scalarop": "oQ.scalarop(op, p1, scalar, p2)",
    "he_double_rns_scalarop": "oQ.{Add,Sub,Mul}DoubleRNSScalar[ThenAdd](p1, s0, s1[, p2])",
    "he_mul_by_vector_montgomery": "oQ.MulByVectorMontgomery(p1, vector[0], [p2])",
    "he_rescale_polys": "oQ.DivRoundByLastModulusManyNTT(nb, p0[i]) per pair",
    "he_automorphism_ntt_with_index": "oQ.AutomorphismNTTWithIndex(pin, oQ.AutomorphismNTTIndex(gal))",
    "he_automorphism_ntt_with_index_then_add_lazy": "oQ.AutomorphismNTTWithIndexThenAddLazy(pin, index, pout)",
    "he_automorphism": "oQ.Automorphism(pin, gal)",
    "he_modup_q_to_p": "O.BasisExtender.ModUpQtoP", "he_modup_p_to_q": "O.BasisExtender.ModUpPtoQ",
    "he_moddown_qp_to_q": "O.BasisExtender.ModDownQPtoQ", "he_moddown_qp_to_q_ntt": "O.BasisExtender.ModDownQPtoQNTT",
    "he_moddown_qp_to_p": "O.BasisExtender.ModDownQPtoP", "he_eval_moddown_qp_to_q_ntt": "O.BasisExtender.ModDownQPtoQNTT",
    "he_decompose_and_split": "O.Decomposer.DecomposeAndSplit (the digit's own limbs of p1Q are not written)",
    "he_gadget_product_lazy": "O.Evaluator.GadgetProductLazy", "he_gadget_product_hoisted_lazy": "O.Evaluator.GadgetProductHoistedLazy",
    "he_gadget_product_hoisted_lazy_digits": "O.Evaluator.GadgetProductHoistedLazy (all digits)",
    "he_moddown": "O.Evaluator.ModDown", "he_gadget_product": "O.Evaluator.GadgetProduct",
    "he_gadget_product_hoisted": "O.Evaluator.GadgetProductHoisted", "he_relinearize": "O.Evaluator.Relinearize",
    "he_automorphism_ct": "O.Evaluator.Automorphism", "he_automorphism_hoisted": "O.Evaluator.AutomorphismHoisted",
    "he_automorphism_hoisted_lazy": "O.Evaluator.AutomorphismHoistedLazy",
    "he_ckks_mul_relin": "O.Evaluator.CKKSMulRelin", "he_bgv_mul_relin": "O.Evaluator.BGVMulRelin",
    "he_centered_lift": "oracle.circuits._centered_lift of src limb 0 into dstQ limbs first_q.. and dstP",
    "he_decomp_fill": "no polynomial output: every operand unchanged",
    "he_lintrans_mul_sum": "Reduce(out_k + sum_i MulCoeffsMontgomery(pt_i, AutomorphismNTTWithIndex?(ct_i[k]))) on oQ and oP",
    "he_lintrans_giant_step": "O.Evaluator.GadgetProductLazy, ringQP Add of (addQ, addP) to component 0, AutomorphismNTTWithIndex"
                              "[ThenAddLazy] into (c_kQ, c_kP)",
}
for _n, _r in ROWS.items():
    _r.oracle = _ORACLE.get(_n, "oQ." + _r.wrapper.split("(")[0].split(".")[-1].replace("ABI ", "") + " on the pre-call words")
