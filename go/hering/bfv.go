package hering

/*
#include "hering_bfv.h"
*/
import "C"

import (
	"fmt"
	"runtime"

	"github.com/tuneinsight/lattigo/v6/core/rlwe"
	"github.com/tuneinsight/lattigo/v6/schemes/bgv"
)

// ScaleInvariantEvaluator mirrors the BFV-style multiplication of bgv.Evaluator (schemes/bgv/evaluator.go:705-1071) on the device:
// MulScaleInvariant[New] and MulRelinScaleInvariant[New] for ciphertext operands of degree 1 are ONE native call each
// (he_bfv_mul_relin: modUpAndNTT, tensorLowDeg, quantize and the relinearisation).  Degree-0 operands, plaintext vectors and
// scalars take the reference's own branches (tensorStandard :718, :749, :819, :852; Mul :754, :857): they are delegated to the
// reference evaluator `Host` and the result's twin is refreshed, as SchemeEvaluator does for host-side operands.
type ScaleInvariantEvaluator struct {
	*Evaluator                // the device evaluator of the parameters (RingQ, RingP), its twins and its key cache
	Host       *bgv.Evaluator // the reference evaluator, for the operands that are encoded on the host
	params     bgv.Parameters
	h          Handle
	ringQMul   *Ring // Parameters.RingQMul() on the device: kept alive with the handle
	levelQMul  []int
}

// NewScaleInvariantEvaluator: newEvaluatorPrecomp (evaluator.go:38-70) on the device.
func NewScaleInvariantEvaluator(eval *Evaluator, params bgv.Parameters, host *bgv.Evaluator) (*ScaleInvariantEvaluator, error) {
	rm, err := NewRing(eval.ctx, params.RingQMul())
	if err != nil {
		return nil, err
	}
	s := &ScaleInvariantEvaluator{Evaluator: eval, Host: host, params: params, ringQMul: rm}
	if err = lockedCall(func() C.int {
		return C.he_bfv_evaluator_create(eval.h, rm.h, C.uint64_t(params.PlaintextModulus()), &s.h)
	}, rm); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(s, func(s *ScaleInvariantEvaluator) { C.he_bfv_evaluator_destroy(s.h) })
	for level := 0; level <= params.MaxLevel(); level++ {
		var lm C.int
		if err = lockedCall(func() C.int { return C.he_bfv_level_qmul(s.h, C.int(level), &lm) }); err != nil {
			return nil, err
		}
		s.levelQMul = append(s.levelQMul, int(lm))
	}
	return s, nil
}

// LevelQMul: evaluatorBase.levelQMul (evaluator.go:33).
func (s *ScaleInvariantEvaluator) LevelQMul() []int { return s.levelQMul }

// host runs f on the reference evaluator and refreshes the twins of the result
func (s *ScaleInvariantEvaluator) host(f func() error, op0, opOut *rlwe.Ciphertext) error {
	if s.Host == nil {
		return fmt.Errorf("cannot MulInvariant: operand is not a ciphertext of degree 1 and no reference evaluator was given")
	}
	if err := s.DownloadCiphertext(op0); err != nil {
		return err
	}
	if err := f(); err != nil {
		return err
	}
	for _, v := range opOut.Value {
		if err := s.Upload(s.RingQ, v); err != nil {
			return err
		}
	}
	return nil
}

// tensor: tensorScaleInvariant (evaluator.go:898-978) on the twins of ct0, ct1 and opOut
func (s *ScaleInvariantEvaluator) tensor(ct0, ct1 *rlwe.Ciphertext, relin bool, opOut *rlwe.Ciphertext) error {
	if ct0.Degree() != 1 || ct1.Degree() != 1 {
		return fmt.Errorf("input elements total degree cannot be larger than 2")
	}
	level := minLevel(ct0, ct1, opOut) // InitOutputBinaryOp (:709, :810)
	var in [4]*Poly
	var err error
	for i := 0; i < 4; i++ {
		src := ct0
		if i >= 2 {
			src = ct1
		}
		if in[i], err = s.twin(s.RingQ, src.Value[i&1], true); err != nil {
			return err
		}
	}
	degree := 2
	var rlk Handle
	if relin {
		key, err := s.keys.GetRelinearizationKey()
		if err != nil {
			return fmt.Errorf("cannot TensorInvariant: %w", err)
		}
		k, err := s.evk(&key.GadgetCiphertext)
		if err != nil {
			return err
		}
		rlk, degree = k.h, 1
	}
	opOut.Resize(degree, level)
	var out [3]Handle
	for i := 0; i <= degree; i++ {
		o, err := s.twin(s.RingQ, opOut.Value[i], false)
		if err != nil {
			return err
		}
		out[i] = o.h
	}
	// (the same ciphertext twice has the same twins: the library takes its squaring branch, :929)
	if err = lockedCall(func() C.int {
		return C.he_bfv_mul_relin(s.h, C.int(level), in[0].h, in[1].h, in[2].h, in[3].h, rlk, out[0], out[1], out[2])
	}, in[0], in[1], in[2], in[3]); err != nil {
		return err
	}
	scale := bgv.MulScaleInvariant(s.params, ct0.Scale, ct1.Scale, level) // :975, :983
	*opOut.MetaData = *ct0.MetaData
	opOut.Scale = scale
	return nil
}

// MulScaleInvariant: evaluator.go:705.  opOut = op0 x op1 * (t / Q) of degree 2, not relinearised.
// Staleness: inputs are read from their device twins (uploaded on first sight only -- call Upload after a host-side change);
// outputs are written on the device only (Download / Sync before reading them on the host).
func (s *ScaleInvariantEvaluator) MulScaleInvariant(op0 *rlwe.Ciphertext, op1 rlwe.Operand, opOut *rlwe.Ciphertext) error {
	if c1, ok := op1.(*rlwe.Ciphertext); ok && c1.Degree() != 0 {
		if err := s.tensor(op0, c1, false, opOut); err != nil {
			return fmt.Errorf("cannot MulInvariant: %w", err)
		}
		return nil
	}
	return s.host(func() error { return s.Host.MulScaleInvariant(op0, op1, opOut) }, op0, opOut)
}

// MulScaleInvariantNew: evaluator.go:778.
func (s *ScaleInvariantEvaluator) MulScaleInvariantNew(op0 *rlwe.Ciphertext, op1 rlwe.Operand) (*rlwe.Ciphertext, error) {
	var opOut *rlwe.Ciphertext
	if c1, ok := op1.(*rlwe.Ciphertext); ok {
		level := op0.Level()
		if c1.Level() < level {
			level = c1.Level()
		}
		opOut = bgv.NewCiphertext(s.params, op0.Degree()+c1.Degree(), level)
	} else {
		opOut = bgv.NewCiphertext(s.params, op0.Degree(), op0.Level())
	}
	return opOut, s.MulScaleInvariant(op0, op1, opOut)
}

// MulRelinScaleInvariant: evaluator.go:806.  The relinearisation key is the one of the evaluator's key set.
// Staleness: as MulScaleInvariant.
func (s *ScaleInvariantEvaluator) MulRelinScaleInvariant(op0 *rlwe.Ciphertext, op1 rlwe.Operand, opOut *rlwe.Ciphertext) error {
	if c1, ok := op1.(*rlwe.Ciphertext); ok && c1.Degree() != 0 {
		if err := s.tensor(op0, c1, true, opOut); err != nil {
			return fmt.Errorf("cannot MulRelinInvariant: %w", err)
		}
		return nil
	}
	return s.host(func() error { return s.Host.MulRelinScaleInvariant(op0, op1, opOut) }, op0, opOut)
}

// MulRelinScaleInvariantNew: evaluator.go:883.
func (s *ScaleInvariantEvaluator) MulRelinScaleInvariantNew(op0 *rlwe.Ciphertext, op1 rlwe.Operand) (*rlwe.Ciphertext, error) {
	var opOut *rlwe.Ciphertext
	if c1, ok := op1.(*rlwe.Ciphertext); ok {
		level := op0.Level()
		if c1.Level() < level {
			level = c1.Level()
		}
		opOut = bgv.NewCiphertext(s.params, 1, level)
	} else {
		opOut = bgv.NewCiphertext(s.params, op0.Degree(), op0.Level())
	}
	if err := s.MulRelinScaleInvariant(op0, op1, opOut); err != nil {
		return nil, fmt.Errorf("cannot MulRelinInvariantNew: %w", err)
	}
	return opOut, nil
}
