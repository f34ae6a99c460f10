package hering

/*
#include "hering_ringpack.h"
*/
import "C"

import (
	"fmt"

	"github.com/tuneinsight/lattigo/v6/core/rlwe"
)

// RingPackingEvaluator serves rlwe.RingPackingEvaluator's Split and Merge (core/rlwe/ring_packing.go:173-228, :376-426) from
// device evaluators, one per ring degree, and the reference's ring-switching keys.  NTT-domain ciphertexts, standard rings.
// The step wrappers below (XPow2NTT, SplitNTT, MergeNTT, ExpandStep, PackPre, PackPost) work on device twins and are what an
// Expand / Pack loop is built from.
type RingPackingEvaluator struct {
	*rlwe.RingPackingEvaluationKey
	Evaluators map[int]*Evaluator
}

// NewRingPackingEvaluator wraps one device evaluator per degree of evk.Parameters.
func NewRingPackingEvaluator(evk *rlwe.RingPackingEvaluationKey, evaluators map[int]*Evaluator) *RingPackingEvaluator {
	return &RingPackingEvaluator{RingPackingEvaluationKey: evk, Evaluators: evaluators}
}

func (r *RingPackingEvaluator) halves(evalN *Evaluator, ct *rlwe.Ciphertext, upload bool) (out [2]*Poly, err error) {
	if ct == nil {
		return
	}
	rHalf, err := evalN.ringOfDegree(evalN.RingQ.N() / 2)
	if err != nil {
		return
	}
	for i := range out {
		if out[i], err = evalN.twin(rHalf, ct.Value[i], upload); err != nil {
			return
		}
	}
	return
}

func optHandle(p *Poly) Handle {
	if p == nil {
		return 0
	}
	return p.h
}

// Split: core/rlwe/ring_packing.go:173-228.  ctN = ctEvenNHalf(Y) + X ctOddNHalf(Y), Y = X^2; ctOddNHalf may be nil.  One key
// switch and one streaming launch on the device.  Same staleness rules as Relinearize.
func (r *RingPackingEvaluator) Split(ctN, ctEvenNHalf, ctOddNHalf *rlwe.Ciphertext) error {
	if r.MinLogN() == r.MaxLogN() {
		return fmt.Errorf("method is not supported when eval.MinLogN() == eval.MaxLogN()")
	}
	if ctN.LogN() <= r.MinLogN() {
		return fmt.Errorf("ctN.Log() must be greater than eval.MinLogN()")
	}
	if ctEvenNHalf == nil {
		return fmt.Errorf("ctEvenNHalf cannot be nil")
	}
	if ctEvenNHalf.LogN() != ctN.LogN()-1 {
		return fmt.Errorf("ctEvenNHalf.LogN() must be equal to ctN.LogN()-1")
	}
	if ctOddNHalf != nil && ctOddNHalf.LogN() != ctN.LogN()-1 {
		return fmt.Errorf("ctOddNHalf.LogN() must be equal to ctN.LogN()-1")
	}
	LogN := ctN.LogN()
	evalN := r.Evaluators[LogN]
	k, err := evalN.evk(&r.RingSwitchingKeys[LogN][LogN-1].GadgetCiphertext)
	if err != nil {
		return err
	}
	var in [2]*Poly
	for i := range in {
		if in[i], err = evalN.twin(evalN.RingQ, ctN.Value[i], true); err != nil {
			return err
		}
	}
	even, err := r.halves(evalN, ctEvenNHalf, false)
	if err != nil {
		return err
	}
	odd, err := r.halves(evalN, ctOddNHalf, false)
	if err != nil {
		return err
	}
	level := ctN.Level()
	odd0, odd1 := optHandle(odd[0]), optHandle(odd[1])
	if err = lockedCall(func() C.int {
		return C.he_ringpack_split(evalN.h, C.int(level), in[0].h, in[1].h, k.h, even[0].h, even[1].h, odd0, odd1)
	}); err != nil {
		return err
	}
	*ctEvenNHalf.MetaData = *ctN.MetaData
	ctEvenNHalf.LogDimensions.Cols--
	if ctOddNHalf != nil {
		*ctOddNHalf.MetaData = *ctN.MetaData
		ctOddNHalf.LogDimensions.Cols--
	}
	return nil
}

// Merge: core/rlwe/ring_packing.go:376-426.  ctOddNHalf may be nil.
func (r *RingPackingEvaluator) Merge(ctEvenNHalf, ctOddNHalf, ctN *rlwe.Ciphertext) error {
	if r.MinLogN() == r.MaxLogN() {
		return fmt.Errorf("method is not supported when eval.MinLogN() == eval.MaxLogN()")
	}
	if ctEvenNHalf == nil {
		return fmt.Errorf("ctEvenNHalf cannot be nil")
	}
	if ctEvenNHalf.LogN() >= r.MaxLogN() {
		return fmt.Errorf("ctEvenNHalf.LogN() must be smaller than eval.MaxLogN()")
	}
	if ctN.LogN() != ctEvenNHalf.LogN()+1 {
		return fmt.Errorf("ctN.LogN() must be equal to ctEvenNHalf.LogN()+1")
	}
	if ctOddNHalf != nil && ctEvenNHalf.LogN() != ctOddNHalf.LogN() {
		return fmt.Errorf("ctEvenNHalf.LogN() and ctOddNHalf.LogN() must be equal")
	}
	LogN := ctN.LogN()
	evalN := r.Evaluators[LogN]
	k, err := evalN.evk(&r.RingSwitchingKeys[LogN-1][LogN].GadgetCiphertext)
	if err != nil {
		return err
	}
	even, err := r.halves(evalN, ctEvenNHalf, true)
	if err != nil {
		return err
	}
	odd, err := r.halves(evalN, ctOddNHalf, true)
	if err != nil {
		return err
	}
	var out [2]*Poly
	for i := range out {
		if out[i], err = evalN.twin(evalN.RingQ, ctN.Value[i], false); err != nil {
			return err
		}
	}
	level := ctN.Level()
	odd0, odd1 := optHandle(odd[0]), optHandle(odd[1])
	if err = lockedCall(func() C.int {
		return C.he_ringpack_merge(evalN.h, C.int(level), even[0].h, even[1].h, odd0, odd1, k.h, out[0].h, out[1].h)
	}); err != nil {
		return err
	}
	*ctN.MetaData = *ctEvenNHalf.MetaData
	ctN.LogDimensions.Cols++
	return nil
}

// XPow2NTT: GenXPow2NTT(ring.AtLevel(level), logN, div)[i] (core/rlwe/ring_packing.go:772-810) into a device polynomial.
func XPow2NTT(r *Ring, level, i int, div bool, out *Poly) error {
	d := 0
	if div {
		d = 1
	}
	return lockedCall(func() C.int { return C.he_ring_xpow2_ntt(r.h, C.int(level), C.int(i), C.int(d), out.h) }, r, out)
}

// SplitNTT: the ring maps of Split on one polynomial of degree N (outOdd may be nil).
func SplitNTT(ringLarge *Ring, level int, in, outEven, outOdd *Poly) error {
	odd := optHandle(outOdd)
	return lockedCall(func() C.int { return C.he_ring_split_ntt(ringLarge.h, C.int(level), in.h, outEven.h, odd) }, ringLarge, in, outEven, outOdd)
}

// MergeNTT: the ring maps of Merge on one polynomial (inOdd may be nil: the replication of inEven).
func MergeNTT(ringLarge *Ring, level int, inEven, inOdd, out *Poly) error {
	odd := optHandle(inOdd)
	return lockedCall(func() C.int { return C.he_ring_merge_ntt(ringLarge.h, C.int(level), inEven.h, odd, out.h) }, ringLarge, inEven, inOdd, out)
}

// ExpandStep: Expand's inner step at n = 2^k (core/rlwe/ring_packing.go:528-559) over batched device ciphertexts.
func ExpandStep(r *Ring, level, k int, sumOnly bool, in, tmp, out [2]*Poly) error {
	s := 0
	if sumOnly {
		s = 1
	}
	return lockedCall(func() C.int {
		return C.he_ringpack_expand_step(r.h, C.int(level), C.int(k), C.int(s), in[0].h, in[1].h, tmp[0].h, tmp[1].h, out[0].h, out[1].h)
	}, r, in, tmp, out)
}

func pairHandles(a, b [][2]*Poly) (a0, a1, b0, b1 []Handle) {
	for z := range a {
		a0, a1 = append(a0, optHandle(a[z][0])), append(a1, optHandle(a[z][1]))
		b0, b1 = append(b0, optHandle(b[z][0])), append(b1, optHandle(b[z][1]))
	}
	return
}

// PackPre: Pack's inner step before the automorphism (core/rlwe/ring_packing.go:697-722) over the pairs (a[z], b[z]); an absent
// ciphertext is [2]*Poly{nil, nil}.  t: the batched T of len(a) entries.
func PackPre(r *Ring, level, k int, a, b [][2]*Poly, t [2]*Poly) error {
	if len(a) == 0 || len(a) != len(b) {
		return fmt.Errorf("hering: PackPre: %d / %d pairs", len(a), len(b))
	}
	a0, a1, b0, b1 := pairHandles(a, b)
	return lockedCall(func() C.int {
		return C.he_ringpack_pack_pre(r.h, C.int(level), C.int(k), C.int(len(a0)), &a0[0], &a1[0], &b0[0], &b1[0], t[0].h, t[1].h)
	}, r, a, b, t)
}

// PackPost: ... and after it (core/rlwe/ring_packing.go:744-764).
func PackPost(r *Ring, level int, a, b [][2]*Poly, t [2]*Poly) error {
	if len(a) == 0 || len(a) != len(b) {
		return fmt.Errorf("hering: PackPost: %d / %d pairs", len(a), len(b))
	}
	a0, a1, b0, b1 := pairHandles(a, b)
	return lockedCall(func() C.int {
		return C.he_ringpack_pack_post(r.h, C.int(level), C.int(len(a0)), &a0[0], &a1[0], &b0[0], &b1[0], t[0].h, t[1].h)
	}, r, a, b, t)
}
