package hering

/*
#include "hering_rgsw.h"
*/
import "C"

import (
	"fmt"

	"github.com/tuneinsight/lattigo/v6/core/rgsw"
	"github.com/tuneinsight/lattigo/v6/core/rlwe"
)

// RGSWEvaluator serves rgsw.Evaluator.ExternalProduct (core/rgsw/evaluator.go:39-82) from a device evaluator.  NTT-domain
// ciphertexts; the two gadget ciphertexts of an RGSW ciphertext become two device keys (cached like every evaluation key).
type RGSWEvaluator struct {
	*Evaluator
}

// NewRGSWEvaluator wraps a device evaluator.
func NewRGSWEvaluator(e *Evaluator) *RGSWEvaluator {
	return &RGSWEvaluator{Evaluator: e}
}

// ExternalProduct: opOut = (<op0, op1[0]>, <op0, op1[1]>), RLWE x RGSW -> RLWE, at the levels of op1.  opOut may be op0.  Same
// staleness rules as Relinearize.
func (r *RGSWEvaluator) ExternalProduct(op0 *rlwe.Ciphertext, op1 *rgsw.Ciphertext, opOut *rlwe.Ciphertext) error {
	if op0.Degree() != 1 || opOut.Degree() != 1 {
		return fmt.Errorf("cannot ExternalProduct: input and output Ciphertext must be of degree 1")
	}
	if !op0.IsNTT {
		return fmt.Errorf("cannot ExternalProduct: hering serves NTT-domain ciphertexts")
	}
	e := r.Evaluator
	k0, err := e.evk(&op1.Value[0])
	if err != nil {
		return err
	}
	k1, err := e.evk(&op1.Value[1])
	if err != nil {
		return err
	}
	var in, out [2]*Poly
	for i := range in {
		if in[i], err = e.twin(e.RingQ, op0.Value[i], true); err != nil {
			return err
		}
	}
	for i := range out {
		if out[i], err = e.twin(e.RingQ, opOut.Value[i], false); err != nil {
			return err
		}
	}
	if err = lockedCall(func() C.int {
		return C.he_rgsw_external_product(e.h, in[0].h, in[1].h, k0.h, k1.h, out[0].h, out[1].h)
	}); err != nil {
		return err
	}
	*opOut.MetaData = *op0.MetaData
	return nil
}
