"""The aliasing table (tests/aliasing_table.py) against include/hering.h, on the host: every entry point with two or more
polynomial handle parameters has a row with the same parameter names, no row names an entry the header does not declare, and
every row marks output/output pairs and written Q/P cross pairs as rejected."""
import itertools
import os
import re

import pytest

from tests import aliasing_table as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hering.h")

# handles that are not polynomials: rings, basis extenders, evaluators, keys, index tables, hoisting buffers, contexts,
# communicators and graphs
_NOT_POLY = re.compile(r"(ring\w*|be|eval|evk|rlk|gk|key|index|decomp|ctx|comm|graph)")


def poly_entries(text: str) -> dict:
    """{entry point: [polynomial handle parameters in order]} for the prototypes with two or more of them"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = {}
    for name, args in re.findall(r"\bint\s+(he_\w+)\s*\(([^;{)]*)\)\s*;", text):
        polys = []
        for a in args.split(","):
            m = re.fullmatch(r"\s*(const\s+)?he_handle\s*(\*)?\s*(\w+)\s*", a)
            if not m:
                continue
            const, ptr, pname = m.groups()
            if ptr and not const:  # a handle the call creates
                continue
            if _NOT_POLY.fullmatch(pname):
                continue
            polys.append(pname)
        if len(polys) >= 2:
            out[name] = polys
    return out


def _header():
    with open(HEADER) as f:
        return f.read()


def test_table_rows_are_the_header_entry_points():
    entries = poly_entries(_header())
    assert len(entries) > 50, sorted(entries)  # the parser found the prototypes
    missing = sorted(set(entries) - set(T.ROWS))
    extra = sorted(set(T.ROWS) - set(entries))
    assert not missing, f"entry points of include/hering.h without a row in tests/aliasing_table.py: {missing}"
    assert not extra, f"rows of tests/aliasing_table.py that include/hering.h does not declare: {extra}"
    for name, params in entries.items():
        assert list(T.ROWS[name].params) == params, (name, params, list(T.ROWS[name].params))


def test_a_new_two_poly_prototype_needs_a_row():
    text = _header().replace("#ifdef __cplusplus\n}", "int he_dummy_op(he_handle ring, int level, he_handle a, he_handle b);\n#ifdef __cplusplus\n}")
    assert "he_dummy_op" in poly_entries(text)
    assert "he_dummy_op" not in T.ROWS


# The in-place forms, written out by hand (hering.h, Conventions) independently of the roles in tests/aliasing_table.py: the
# (output, input) pairs each row must accept.  "*": every output with every input (coefficient-wise ops, Relinearize,
# Automorphism on ciphertexts, MulRelin).  Rows not listed accept no (output, input) pair.
_COEFF = ("he_ntt", "he_ntt_lazy", "he_intt", "he_intt_lazy", "he_binop", "he_unop", "he_scalarop", "he_mul_rns_scalar_montgomery",
          "he_add_scalar_bigint", "he_sub_scalar_bigint", "he_mul_scalar_bigint", "he_mul_scalar_bigint_then_add", "he_double_rns_scalarop",
          "he_shift", "he_mult_by_monomial", "he_add", "he_sub", "he_mul_coeffs_montgomery", "he_mul_coeffs_montgomery_then_add",
          "he_mul_coeffs_montgomery_lazy", "he_mul_coeffs_montgomery_lazy_then_add_lazy", "he_neg", "he_reduce", "he_mform", "he_imform",
          "he_div_round_by_last_modulus_ntt", "he_div_round_by_last_modulus", "he_div_floor_by_last_modulus_ntt",
          "he_div_floor_by_last_modulus", "he_div_round_by_last_modulus_many_ntt", "he_div_round_by_last_modulus_many",
          "he_div_floor_by_last_modulus_many_ntt", "he_div_floor_by_last_modulus_many")
IN_PLACE = {**{n: "*" for n in _COEFF},
            "he_poly_copy": {("dst", "src")},
            "he_mul_by_vector_montgomery": {("p2", "p1")},
            "he_rescale_polys": {("p1", "p0")},
            "he_moddown_qp_to_q": {("p2Q", "p1Q")}, "he_moddown_qp_to_q_ntt": {("p2Q", "p1Q")}, "he_moddown_qp_to_p": {("p2P", "p1P")},
            "he_moddown": {("out0", "c0Q"), ("out1", "c1Q")},
            "he_eval_moddown_qp_to_q_ntt": {("p2Q", "p1Q")},
            "he_gadget_product": {("out0", "cx"), ("out1", "cx")},
            "he_relinearize": "*", "he_automorphism_ct": "*", "he_automorphism_hoisted": "*",
            "he_automorphism_hoisted_lazy": {("c0Q", "in0"), ("c1Q", "in0")},
            "he_ckks_mul_relin": "*", "he_bgv_mul_relin": "*",
            "he_centered_lift": {("dstQ", "src")}}
# (output, output) and written Q/P cross pairs every row must reject, written out for the rows that have them
MUST_REJECT = {
    "he_modup_q_to_p": {("polP", "polQ")}, "he_modup_p_to_q": {("polQ", "polP")},
    "he_moddown_qp_to_q": {("p2Q", "p1P")}, "he_moddown_qp_to_q_ntt": {("p2Q", "p1P")}, "he_moddown_qp_to_p": {("p2P", "p1Q")},
    "he_decompose_and_split": {("p1Q", "p1P"), ("p1Q", "p0Q"), ("p1P", "p0Q")},
    "he_gadget_product_lazy": {("c0Q", "c1Q"), ("c0P", "c1P"), ("c0Q", "c0P"), ("c0Q", "c1P"), ("c0P", "c1Q"), ("c1Q", "c1P"),
                               ("c0P", "cx"), ("c1P", "cx"), ("c0Q", "cx"), ("c1Q", "cx")},
    "he_gadget_product": {("out0", "out1")}, "he_gadget_product_hoisted": {("out0", "out1")},
    "he_moddown": {("out0", "c0P"), ("out1", "c1P"), ("out0", "out1"), ("out0", "c1Q"), ("out1", "c0Q")},
    "he_eval_moddown_qp_to_q_ntt": {("p2Q", "p1P")},
    "he_relinearize": {("out0", "out1")}, "he_automorphism_ct": {("out0", "out1")},
    "he_automorphism_hoisted_lazy": {("c0P", "in0"), ("c1P", "in0"), ("c0Q", "c1Q"), ("c0P", "c1P")},
    "he_ckks_mul_relin": {("out0", "out1"), ("out1", "out2")},
    "he_centered_lift": {("dstP", "src"), ("dstQ", "dstP")},
    "he_lintrans_giant_step": {("c0Q", "c1Q"), ("c0Q", "c0P"), ("c0P", "cx"), ("c1Q", "addQ"), ("c1P", "addP"), ("c0Q", "addP")},
    "he_lintrans_mul_sum": {("out0Q", "ptQ"), ("out1P", "ptP"), ("out0Q", "ct0P"), ("out0P", "ct1Q"), ("out0Q", "out1Q")},
    "he_automorphism": {("pout", "pin")}, "he_automorphism_ntt_with_index": {("pout", "pin")},
    "he_automorphism_ntt_with_index_then_add_lazy": {("pout", "pin")},
    "he_poly_copy_batch": {("dst", "src")},
}


@pytest.mark.parametrize("name", sorted(T.ROWS))
def test_row_matches_the_hand_written_rule(name):
    """the table's verdicts against the rule as the header states it, written out above"""
    row = T.ROWS[name]
    want = IN_PLACE.get(name, set())
    for o in row.params:
        for i in row.params:
            if not row.written(o) or row.written(i):
                continue
            allowed = want == "*" and row.side(o) == row.side(i) or want != "*" and (o, i) in want
            assert row.verdict(o, i) == ("accept" if allowed else "reject"), (name, o, i)
    for a, b in MUST_REJECT.get(name, set()):
        assert row.verdict(a, b) == "reject" and row.verdict(b, a) == "reject", (name, a, b)


@pytest.mark.parametrize("name", sorted(T.ROWS))
def test_every_row_rejects_output_pairs_and_written_cross_pairs(name):
    row = T.ROWS[name]
    for o, i in row.allowed:
        assert o in row.params and i in row.params, (o, i)
        assert row.written(o) and not row.written(i), (o, i)
        assert row.side(o) == row.side(i), (o, i)
    for a, b in itertools.combinations_with_replacement(row.params, 2):
        if a == b and a not in row.arrays:
            continue
        v = row.verdict(a, b)
        if row.written(a) and row.written(b):
            assert v == "reject", (a, b)
        elif (row.written(a) or row.written(b)) and row.side(a) != row.side(b):
            assert v == "reject", (a, b)
        elif not row.written(a) and not row.written(b):
            assert v == "accept", (a, b)
    for groups in T.patterns(row):
        for g in groups:
            outs = [x for x in g if row.written(T.base(x))]
            if len(outs) > 1:
                assert T.pattern_verdict(row, groups) == "reject", groups


def test_the_in_place_forms_the_header_promises_stay_accepted():
    R = T.ROWS
    for name in ("he_ntt", "he_intt", "he_binop", "he_unop", "he_scalarop", "he_shift", "he_mult_by_monomial",
                 "he_div_round_by_last_modulus_many_ntt", "he_double_rns_scalarop", "he_mul_scalar_bigint_then_add"):
        assert all(T.pattern_verdict(R[name], g) == "accept" for g in T.patterns(R[name])), name
    assert R["he_moddown_qp_to_q_ntt"].verdict("p2Q", "p1Q") == "accept"
    assert R["he_eval_moddown_qp_to_q_ntt"].verdict("p2Q", "p1Q") == "accept"
    assert R["he_gadget_product"].verdict("out0", "cx") == "accept"
    for name, outs, ins in (("he_relinearize", ("out0", "out1"), ("in0", "in1", "in2")),
                            ("he_automorphism_ct", ("out0", "out1"), ("in0", "in1")),
                            ("he_ckks_mul_relin", ("out0", "out1"), ("a0", "a1", "b0", "b1"))):
        for o in outs:
            for i in ins:
                assert R[name].verdict(o, i) == "accept", (name, o, i)
    # MulRelin(res, res, res) and the crossed outputs
    assert T.pattern_verdict(R["he_ckks_mul_relin"], [("a0", "b0", "out0"), ("a1", "b1", "out1")]) == "accept"
    # already rejected: ring automorphisms in place, the giant step and lintrans outputs on an input
    assert R["he_automorphism"].verdict("pout", "pin") == "reject"
    assert all(R["he_lintrans_giant_step"].verdict(o, i) == "reject" for o in ("c0Q", "c0P", "c1Q", "c1P") for i in ("cx", "addQ", "addP"))
    # he_rescale_polys: a pair in place, never across pairs
    rp = R["he_rescale_polys"]
    assert T.pattern_verdict(rp, [("p0[0]", "p1[0]")]) == "accept"
    assert T.pattern_verdict(rp, [("p0[1]", "p1[0]")]) == "reject"
    assert T.pattern_verdict(rp, [("p1[0]", "p1[1]")]) == "reject"
