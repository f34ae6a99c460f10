package hering

/*
#include "hering_ringswitch.h"
*/
import "C"

import (
	"fmt"
	"math/bits"

	"github.com/tuneinsight/lattigo/v6/core/rlwe"
	"github.com/tuneinsight/lattigo/v6/ring"
)

// ringOfDegree returns the device ring of degree n over the evaluator's Q moduli: RingQ itself at n = N, a twin of smaller
// degree (the same moduli, the same ring type) otherwise, created on first use and shared with the ShallowCopy's.
func (e *Evaluator) ringOfDegree(n int) (*Ring, error) {
	if n == e.RingQ.N() {
		return e.RingQ, nil
	}
	logN := bits.Len(uint(n)) - 1
	sm := e.sharedMu()
	sm.Lock()
	defer sm.Unlock()
	if r, ok := e.small[logN]; ok {
		return r, nil
	}
	host, err := ring.NewRingFromType(n, e.params.RingQ().ModuliChain(), e.params.RingQ().Type())
	if err != nil {
		return nil, fmt.Errorf("hering: ring of degree %d: %w", n, err)
	}
	r, err := NewRing(e.ctx, host)
	if err != nil {
		return nil, err
	}
	e.small[logN] = r
	return r, nil
}

// ApplyEvaluationKey: core/rlwe/evaluator_evaluationkey.go:36-106 (NTT domain).  ctIn and opOut of the evaluator's degree, or one of
// them of a smaller degree: n -> N maps ctIn up (SwitchCiphertextRingDegreeNTT) and key-switches, N -> n key-switches and folds the
// result down; the key is of degree N in every case.  Same staleness rules as Relinearize.
func (e *Evaluator) ApplyEvaluationKey(ctIn *rlwe.Ciphertext, evk *rlwe.EvaluationKey, opOut *rlwe.Ciphertext) error {
	if ctIn.Degree() != 1 || opOut.Degree() != 1 {
		return fmt.Errorf("cannot ApplyEvaluationKey: input and output Ciphertext must be of degree 1")
	}
	if !ctIn.IsNTT {
		return fmt.Errorf("cannot ApplyEvaluationKey: hering serves NTT-domain ciphertexts")
	}
	level := ctIn.Level()
	if opOut.Level() < level {
		level = opOut.Level()
	}
	NIn, NOut, N := ctIn.Value[0].N(), opOut.Value[0].N(), e.RingQ.N()
	if NIn < NOut && NOut != N {
		return fmt.Errorf("cannot ApplyEvaluationKey: opOut ring degree does not match evaluator params ring degree")
	}
	if NIn > NOut && NIn != N {
		return fmt.Errorf("cannot ApplyEvaluationKey: ctIn ring degree does not match evaluator params ring degree")
	}
	if NIn == NOut && NIn != N {
		return fmt.Errorf("cannot ApplyEvaluationKey: ctIn and opOut ring degree does not match evaluator params ring degree")
	}
	k, err := e.evk(&evk.GadgetCiphertext)
	if err != nil {
		return err
	}
	rIn, err := e.ringOfDegree(NIn)
	if err != nil {
		return err
	}
	rOut, err := e.ringOfDegree(NOut)
	if err != nil {
		return err
	}
	var in, out [2]*Poly
	for i := range in {
		if in[i], err = e.twin(rIn, ctIn.Value[i], true); err != nil {
			return err
		}
	}
	for i := range out {
		if out[i], err = e.twin(rOut, opOut.Value[i], false); err != nil {
			return err
		}
	}
	if err = lockedCall(func() C.int {
		return C.he_apply_evaluation_key(e.h, C.int(level), in[0].h, in[1].h, k.h, out[0].h, out[1].h)
	}); err != nil {
		return err
	}
	opOut.Resize(1, level)
	*opOut.MetaData = *ctIn.MetaData
	return nil
}

// SwitchCiphertextRingDegreeNTT: core/rlwe/element.go:250 on device twins (limbs 0..min(level)).  ringQLargeDim is required for
// large -> small and may be nil otherwise.
func SwitchCiphertextRingDegreeNTT(ctIn []*Poly, ringQLargeDim *Ring, opOut []*Poly) error {
	var hr Handle
	if ringQLargeDim != nil {
		hr = ringQLargeDim.h
	}
	for i := range opOut {
		level := ctIn[i].limbs - 1
		if opOut[i].limbs-1 < level {
			level = opOut[i].limbs - 1
		}
		a, b := ctIn[i], opOut[i]
		if err := lockedCall(func() C.int { return C.he_switch_ring_degree_ntt(hr, C.int(level), a.h, b.h) }, a, b, ringQLargeDim); err != nil {
			return err
		}
	}
	return nil
}
