package hering

/*
#include "hering_ckks_evaluator.h"
*/
import "C"

// The entries of hering_ckks_evaluator.h: the linear forms of ckks.Evaluator (schemes/ckks/evaluator.go) over every component of a
// ciphertext, and MulRelinThenAdd, one launch each.  The caller plans levels, scales (the reference's own rlwe.Scale serves) and
// the residues of scalars, ratios and scale-ups: every word list holds one residue per limb 0 .. level.

func handleList(ps []*Poly) []Handle {
	out := make([]Handle, len(ps)+1)
	for i, p := range ps {
		out[i] = h(p)
	}
	return out
}

// CKKSAddSub: evaluateInPlace (:221-408) with Ring.Add / Ring.Sub over the components; scaled = 1 / 2: op0 / op1 is first
// multiplied by the integer with the residues ratio.
func (r *Ring) CKKSAddSub(sub bool, op0, op1 []*Poly, scaled int, ratio []uint64, opOut []*Poly) error {
	a, b, o := handleList(op0), handleList(op1), handleList(opOut)
	s := 0
	if sub {
		s = 1
	}
	return lockedCall(func() C.int {
		return C.he_ckks_add(r.h, C.int(r.level), C.int(s), C.int(len(op0)), &a[0], C.int(len(op1)), &b[0], C.int(scaled), u64ptr(ratio), C.int(len(opOut)), &o[0])
	}, op0, op1, opOut)
}

// CKKSScalar: evaluateWithScalar (:410-424); op 0 add, 1 sub, 2 mul, 3 mul-then-add onto opOut (pre: its scale-up, or nil).
func (r *Ring) CKKSScalar(op int, op0 []*Poly, s0, s1, pre []uint64, opOut []*Poly) error {
	a, o := handleList(op0), handleList(opOut)
	return lockedCall(func() C.int {
		return C.he_ckks_scalar(r.h, C.int(r.level), C.int(op), C.int(len(op0)), &a[0], u64ptr(s0), u64ptr(s1), u64ptr(pre), &o[0])
	}, op0, opOut)
}

// CKKSMulPlaintext: the plaintext branches of mulRelin (:842-869) and mulRelinThenAdd (:1158-1170).
func (r *Ring) CKKSMulPlaintext(ct []*Poly, pt *Poly, thenAdd bool, pre []uint64, opOut []*Poly) error {
	a, o := handleList(ct), handleList(opOut)
	t := 0
	if thenAdd {
		t = 1
	}
	return lockedCall(func() C.int {
		return C.he_ckks_mul_pt(r.h, C.int(r.level), C.int(len(ct)), &a[0], h(pt), C.int(t), u64ptr(pre), &o[0])
	}, ct, pt, opOut)
}

// CKKSMulRelinThenAdd: the ciphertext x ciphertext branch of mulRelinThenAdd (:1104-1155); rlk nil: MulThenAdd onto the three
// components of opOut.
func (e *Evaluator) CKKSMulRelinThenAdd(level int, op0, op1 []*Poly, rlk *EvaluationKey, pre []uint64, opOut []*Poly) error {
	var k, o2 Handle
	if rlk != nil {
		k = rlk.h
	} else if len(opOut) > 2 {
		o2 = h(opOut[2])
	}
	return lockedCall(func() C.int {
		return C.he_ckks_mul_relin_then_add(e.h, C.int(level), h(op0[0]), h(op0[1]), h(op1[0]), h(op1[1]), k, u64ptr(pre), h(opOut[0]), h(opOut[1]), o2)
	}, op0, op1, opOut)
}
