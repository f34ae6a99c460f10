package hering

/*
#include "hering_lintrans.h"
*/
import "C"

import (
	"fmt"
	"runtime"
	"sort"
	"unsafe"

	"github.com/tuneinsight/lattigo/v6/circuits/common/lintrans"
	"github.com/tuneinsight/lattigo/v6/core/rlwe"
)

// LinearTransformation is a lintrans.LinearTransformation whose encoded diagonals have device twins and whose evaluation plan
// lives in the library (he_lintrans_create).  The handle reads the twins' words when the transformation is evaluated: after a
// host-side change of a diagonal call Evaluator.Upload on it, as for every other input.
type LinearTransformation struct {
	Host lintrans.LinearTransformation
	h    Handle
	keep []*Poly // the twins of the diagonals, alive with the handle
}

// BSGSIndex: lintrans.BSGSIndex (lintrans.go:344) through the library's restatement.
func BSGSIndex(nonZeroDiags []int, slots, N1 int) (rotN1, rotN2 []int, err error) {
	d := cInts(nonZeroDiags)
	r1, r2 := make([]C.int, len(nonZeroDiags)+1), make([]C.int, len(nonZeroDiags)+1)
	var n1, n2 C.int
	if err = lockedCall(func() C.int {
		return C.he_lintrans_bsgs_index(&d[0], C.int(len(nonZeroDiags)), C.int(slots), C.int(N1), &r1[0], &n1, &r2[0], &n2, nil)
	}); err != nil {
		return
	}
	for i := 0; i < int(n1); i++ {
		rotN1 = append(rotN1, int(r1[i]))
	}
	for i := 0; i < int(n2); i++ {
		rotN2 = append(rotN2, int(r2[i]))
	}
	return
}

// FindBestBSGSRatio: lintrans.FindBestBSGSRatio (lintrans.go:321).
func FindBestBSGSRatio(nonZeroDiags []int, maxN, logMaxRatio int) (N1 int, err error) {
	d := cInts(nonZeroDiags)
	var out C.int
	err = lockedCall(func() C.int {
		return C.he_lintrans_find_best_bsgs_ratio(&d[0], C.int(len(nonZeroDiags)), C.int(maxN), C.int(logMaxRatio), &out)
	})
	return int(out), err
}

// LinTransGaloisElements: lintrans.GaloisElements (lintrans.go:297) on the evaluator's ring.
func (e *Evaluator) LinTransGaloisElements(diags []int, slots, logBSGSRatio int) (galEls []uint64, err error) {
	d := cInts(diags)
	els := make([]uint64, 2*len(diags)+2)
	var n C.size_t
	if err = lockedCall(func() C.int {
		return C.he_lintrans_galois_elements(e.h, &d[0], C.int(len(diags)), C.int(slots), C.int(logBSGSRatio),
			(*C.uint64_t)(unsafe.Pointer(&els[0])), C.size_t(len(els)), &n)
	}); err != nil {
		return
	}
	return els[:int(n)], nil
}

func cInts(v []int) []C.int {
	out := make([]C.int, len(v)+1)
	for i, x := range v {
		out[i] = C.int(x)
	}
	return out
}

// NewLinearTransformation makes the encoded transformation lt resident: the twins of its diagonals (uploaded on first sight) and
// the plan of its evaluation.
func (e *Evaluator) NewLinearTransformation(lt lintrans.LinearTransformation) (*LinearTransformation, error) {
	idx := make([]int, 0, len(lt.Vec))
	for k := range lt.Vec {
		idx = append(idx, k)
	}
	sort.Ints(idx)
	d := &LinearTransformation{Host: lt}
	hq, hp := make([]Handle, len(idx)+1), make([]Handle, len(idx)+1)
	for i, k := range idx {
		q, p, err := e.qp(lt.Vec[k], lt.LevelP, true)
		if err != nil {
			return nil, err
		}
		hq[i], hp[i] = q.h, h(p)
		d.keep = append(d.keep, q, p)
	}
	ci := cInts(idx)
	if err := lockedCall(func() C.int {
		return C.he_lintrans_create(e.h, C.int(lt.LevelQ), C.int(lt.LevelP), C.int(lt.LogDimensions.Cols), C.int(lt.N1), C.int(len(idx)),
			&ci[0], &hq[0], &hp[0], &d.h)
	}); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(d, func(d *LinearTransformation) { C.he_lintrans_destroy(d.h) })
	return d, nil
}

// SetGroup: giant steps per launch of the grouped kernel, 0 (the library's default), 1, 2 or 4.
func (lt *LinearTransformation) SetGroup(G int) error {
	return lockedCall(func() C.int { return C.he_lintrans_set_group(lt.h, C.int(G)) })
}

// LinTransEvaluator is lintrans.Evaluator (lintrans_evaluator.go:12) as ONE native call per EvaluateMany: nothing of the
// reference's loops runs on the host, so no host buffer can be stale in the middle of a product.
type LinTransEvaluator struct {
	*Evaluator
	set  Handle
	keys []*EvaluationKey
}

// NewLinTransEvaluator makes the Galois keys of galEls resident as the key set the evaluations address.
func NewLinTransEvaluator(eval *Evaluator, galEls []uint64) (*LinTransEvaluator, error) {
	gks := make([]*rlwe.GaloisKey, 0, len(galEls))
	for _, g := range galEls {
		if g == 1 {
			continue
		}
		gk, err := eval.CheckAndGetGaloisKey(g)
		if err != nil {
			return nil, fmt.Errorf("cannot NewLinTransEvaluator: %w", err)
		}
		gks = append(gks, gk)
	}
	l := &LinTransEvaluator{Evaluator: eval}
	if len(gks) > 0 {
		var err error
		if l.set, l.keys, err = eval.NewGaloisKeySet(gks); err != nil {
			return nil, err
		}
		runtime.SetFinalizer(l, func(l *LinTransEvaluator) { C.he_galois_keyset_destroy(l.set) })
	}
	return l, nil
}

// EvaluateMany: lintrans_evaluator.go:27.
// Staleness: the input is read from its device twins (uploaded on first sight only -- call Upload after a host-side change);
// outputs are written on the device only (Download / Sync before reading them on the host).
func (l *LinTransEvaluator) EvaluateMany(ctIn *rlwe.Ciphertext, lts []*LinearTransformation, opOut []*rlwe.Ciphertext) error {
	if len(opOut) < len(lts) {
		return fmt.Errorf("output *rlwe.Ciphertext slice is too small")
	}
	if len(lts) == 0 {
		return nil
	}
	in0, err := l.twin(l.RingQ, ctIn.Value[0], true)
	if err != nil {
		return err
	}
	in1, err := l.twin(l.RingQ, ctIn.Value[1], true)
	if err != nil {
		return err
	}
	hl, o0, o1 := make([]Handle, len(lts)), make([]Handle, len(lts)), make([]Handle, len(lts))
	for k, lt := range lts {
		hl[k] = lt.h
		level := ctIn.Level() // :149, :172 / :287, :310: min(opOut.Level(), ctIn.Level(), LevelQ), and opOut is resized to it
		if lt.Host.LevelQ < level {
			level = lt.Host.LevelQ
		}
		if opOut[k].Level() < level {
			level = opOut[k].Level()
		}
		opOut[k].Resize(opOut[k].Degree(), level)
		a, err := l.twin(l.RingQ, opOut[k].Value[0], false)
		if err != nil {
			return err
		}
		b, err := l.twin(l.RingQ, opOut[k].Value[1], false)
		if err != nil {
			return err
		}
		o0[k], o1[k] = a.h, b.h
	}
	if err = lockedCall(func() C.int {
		return C.he_lintrans_evaluate_many(l.h, l.set, C.int(ctIn.Level()), in0.h, in1.h, C.int(len(lts)), &hl[0], &o0[0], &o1[0])
	}, in0, in1); err != nil {
		return fmt.Errorf("cannot EvaluateMany: %w", err)
	}
	for k, lt := range lts {
		*opOut[k].MetaData = *ctIn.MetaData
		opOut[k].Scale = ctIn.Scale.Mul(lt.Host.Scale)
	}
	return nil
}

// Evaluate: lintrans_evaluator.go:122.
func (l *LinTransEvaluator) Evaluate(ctIn *rlwe.Ciphertext, lt *LinearTransformation, opOut *rlwe.Ciphertext) error {
	return l.EvaluateMany(ctIn, []*LinearTransformation{lt}, []*rlwe.Ciphertext{opOut})
}
