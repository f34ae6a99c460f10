package hering

/*
#include "hering_bridge.h"
*/
import "C"

import (
	"fmt"

	"github.com/tuneinsight/lattigo/v6/core/rlwe"
	"github.com/tuneinsight/lattigo/v6/ring"
)

// DomainSwitcher mirrors ckks.DomainSwitcher (schemes/ckks/bridge.go:13-47) on the device: the bridge between the standard CKKS
// domain in Z[X]/(X^N+1) and the conjugate-invariant one in Z[X+X^-1]/(X^N+1), held in compressed form (N/2 words per limb).
type DomainSwitcher struct {
	stdToci, ciToStd *rlwe.EvaluationKey
	ciRing           *Ring // the conjugate-invariant ring of degree N/2 over the evaluator's Q moduli: the twins of the real side
}

// NewDomainSwitcher: ckks.NewDomainSwitcher (bridge.go:25).  eval is the device evaluator of the standard ring of degree N; the
// keys are those of rlwe.KeyGenerator.GenEvaluationKeysForRingSwapNew and either may be nil.
func NewDomainSwitcher(eval *Evaluator, comlexToRealEvk, realToComplexEvk *rlwe.EvaluationKey) (*DomainSwitcher, error) {
	host, err := eval.params.RingQ().ConjugateInvariantRing()
	if err != nil {
		return nil, fmt.Errorf("cannot NewDomainSwitcher because the standard NTT is undefined for params: %s", err)
	}
	r, err := NewRing(eval.ctx, host)
	if err != nil {
		return nil, err
	}
	return &DomainSwitcher{stdToci: comlexToRealEvk, ciToStd: realToComplexEvk, ciRing: r}, nil
}

// call runs one of the two entries on the device twins of ctIn and opOut
func (s *DomainSwitcher) call(eval *Evaluator, toReal bool, level int, ctIn *rlwe.Ciphertext, evk *rlwe.EvaluationKey, opOut *rlwe.Ciphertext) error {
	k, err := eval.evk(&evk.GadgetCiphertext)
	if err != nil {
		return err
	}
	rIn, rOut := s.ciRing, eval.RingQ
	if toReal {
		rIn, rOut = eval.RingQ, s.ciRing
	}
	var in, out [2]*Poly
	for i := range in {
		if in[i], err = eval.twin(rIn, ctIn.Value[i], true); err != nil {
			return err
		}
	}
	for i := range out {
		if out[i], err = eval.twin(rOut, opOut.Value[i], false); err != nil {
			return err
		}
	}
	return lockedCall(func() C.int {
		if toReal {
			return C.he_complex_to_real(eval.h, C.int(level), in[0].h, in[1].h, k.h, out[0].h, out[1].h)
		}
		return C.he_real_to_complex(eval.h, C.int(level), in[0].h, in[1].h, k.h, out[0].h, out[1].h)
	})
}

// ComplexToReal: bridge.go:57-95.  ctIn of degree N, opOut of degree N/2; the scale of opOut is twice that of ctIn.
func (s *DomainSwitcher) ComplexToReal(eval *Evaluator, ctIn, opOut *rlwe.Ciphertext) error {
	if eval.params.RingType() != ring.Standard {
		return fmt.Errorf("cannot ComplexToReal: provided evaluator is not instantiated with RingType ring.Standard")
	}
	level := ctIn.Level()
	if opOut.Level() < level {
		level = opOut.Level()
	}
	if ctIn.Value[0].N() != 2*opOut.Value[0].N() {
		return fmt.Errorf("cannot ComplexToReal: ctIn ring degree must be twice opOut ring degree")
	}
	opOut.Resize(1, level)
	if s.stdToci == nil {
		return fmt.Errorf("cannot ComplexToReal: no realToComplexEvk provided to this DomainSwitcher")
	}
	if err := s.call(eval, true, level, ctIn, s.stdToci, opOut); err != nil {
		return err
	}
	*opOut.MetaData = *ctIn.MetaData
	opOut.Scale = ctIn.Scale.Mul(rlwe.NewScale(2))
	return nil
}

// RealToComplex: bridge.go:104-144.  ctIn of degree N/2, opOut of degree N.
func (s *DomainSwitcher) RealToComplex(eval *Evaluator, ctIn, opOut *rlwe.Ciphertext) error {
	if eval.params.RingType() != ring.Standard {
		return fmt.Errorf("cannot RealToComplex: provided evaluator is not instantiated with RingType ring.Standard")
	}
	level := ctIn.Level()
	if opOut.Level() < level {
		level = opOut.Level()
	}
	if 2*ctIn.Value[0].N() != opOut.Value[0].N() {
		return fmt.Errorf("cannot RealToComplex: opOut ring degree must be twice ctIn ring degree")
	}
	opOut.Resize(1, level)
	if s.ciToStd == nil {
		return fmt.Errorf("cannot RealToComplex: no realToComplexEvk provided to this DomainSwitcher")
	}
	if err := s.call(eval, false, level, ctIn, s.ciToStd, opOut); err != nil {
		return err
	}
	*opOut.MetaData = *ctIn.MetaData
	return nil
}
