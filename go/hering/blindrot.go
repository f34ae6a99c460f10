package hering

/*
#include "hering_blindrot.h"
*/
import "C"

import (
	"fmt"
	"runtime"
	"unsafe"

	"github.com/tuneinsight/lattigo/v6/core/rgsw"
	"github.com/tuneinsight/lattigo/v6/core/rlwe"
)

// BlindRotationKeySet is blindrot.MemBlindRotationEvaluationKeySet (core/rgsw/blindrot/keys.go:32) made resident: the blind
// rotation keys as a table of RGSW ciphertexts and the automorphism keys as a table of Galois keys with their index tables.
type BlindRotationKeySet struct {
	rgswSet   Handle
	galoisSet Handle
	keys      []*EvaluationKey // kept alive with the set
	nLWE      int
}

// NewGaloisKeySet makes the Galois keys resident as one table (he_galois_keyset_create).
func (e *Evaluator) NewGaloisKeySet(gks []*rlwe.GaloisKey) (set Handle, keys []*EvaluationKey, err error) {
	if len(gks) == 0 {
		return 0, nil, fmt.Errorf("cannot NewGaloisKeySet: no key")
	}
	galEls := make([]C.uint64_t, len(gks))
	hs := make([]Handle, len(gks))
	for i, gk := range gks {
		k, err := e.evk(&gk.GadgetCiphertext)
		if err != nil {
			return 0, nil, err
		}
		keys = append(keys, k)
		galEls[i] = C.uint64_t(gk.GaloisElement)
		hs[i] = k.h
	}
	err = lockedCall(func() C.int {
		return C.he_galois_keyset_create(e.h, C.int(len(gks)), &galEls[0], &hs[0], &set)
	}, keys)
	return
}

// NewBlindRotationKeySet makes BlindRotationKeys and AutomorphismKeys resident.
func (e *Evaluator) NewBlindRotationKeySet(brk []*rgsw.Ciphertext, gks []*rlwe.GaloisKey) (*BlindRotationKeySet, error) {
	if len(brk) == 0 {
		return nil, fmt.Errorf("cannot NewBlindRotationKeySet: no blind rotation key")
	}
	ks := &BlindRotationKeySet{nLWE: len(brk)}
	k0 := make([]Handle, len(brk))
	k1 := make([]Handle, len(brk))
	for i, ct := range brk {
		a, err := e.evk(&ct.Value[0])
		if err != nil {
			return nil, err
		}
		b, err := e.evk(&ct.Value[1])
		if err != nil {
			return nil, err
		}
		ks.keys = append(ks.keys, a, b)
		k0[i], k1[i] = a.h, b.h
	}
	if err := lockedCall(func() C.int {
		return C.he_rgsw_keyset_create(e.h, C.int(len(brk)), &k0[0], &k1[0], &ks.rgswSet)
	}, ks.keys); err != nil {
		return nil, err
	}
	set, keys, err := e.NewGaloisKeySet(gks)
	if err != nil {
		C.he_rgsw_keyset_destroy(ks.rgswSet)
		return nil, err
	}
	ks.galoisSet = set
	ks.keys = append(ks.keys, keys...)
	runtime.SetFinalizer(ks, func(s *BlindRotationKeySet) {
		C.he_galois_keyset_destroy(s.galoisSet)
		C.he_rgsw_keyset_destroy(s.rgswSet)
	})
	return ks, nil
}

// BlindRotationEvaluator serves blindrot.Evaluator.BlindRotateCore (core/rgsw/blindrot/evaluator.go:135) from a device
// evaluator.  Evaluate's prologue (the switch to modulus 2N, the accumulator's initial value) stays with the caller.
type BlindRotationEvaluator struct {
	*Evaluator
}

// NewBlindRotationEvaluator wraps a device evaluator.
func NewBlindRotationEvaluator(e *Evaluator) *BlindRotationEvaluator {
	return &BlindRotationEvaluator{Evaluator: e}
}

func (b *BlindRotationEvaluator) twins(ctIn, opOut *rlwe.Ciphertext) (in, out [2]*Poly, err error) {
	e := b.Evaluator
	for i := range in {
		if in[i], err = e.twin(e.RingQ, ctIn.Value[i], true); err != nil {
			return
		}
	}
	for i := range out {
		if out[i], err = e.twin(e.RingQ, opOut.Value[i], false); err != nil {
			return
		}
	}
	return
}

// BlindRotateCore updates acc in place following the schedule of the row a (words mod 2N, one per blind rotation key).
func (b *BlindRotationEvaluator) BlindRotateCore(a []uint64, acc *rlwe.Ciphertext, ks *BlindRotationKeySet) error {
	if acc.Degree() != 1 || !acc.IsNTT {
		return fmt.Errorf("cannot BlindRotateCore: the accumulator is a degree-1 ciphertext in the NTT domain")
	}
	if len(a) == 0 || len(a) > ks.nLWE {
		return fmt.Errorf("cannot BlindRotateCore: %d words for %d blind rotation keys", len(a), ks.nLWE)
	}
	in, _, err := b.twins(acc, acc)
	if err != nil {
		return err
	}
	e := b.Evaluator
	return lockedCall(func() C.int {
		return C.he_blind_rotate_core(e.h, (*C.uint64_t)(unsafe.Pointer(&a[0])), C.int(1), C.int(len(a)), in[0].h, in[1].h, ks.rgswSet, ks.galoisSet)
	}, ks, a)
}

// AutomorphismSelect is rlwe.Evaluator.Automorphism with key sel of the set's Galois keys (-1: a copy); opOut may be ctIn.
func (b *BlindRotationEvaluator) AutomorphismSelect(ctIn *rlwe.Ciphertext, ks *BlindRotationKeySet, sel int32, opOut *rlwe.Ciphertext) error {
	if ctIn.Degree() != 1 || opOut.Degree() != 1 || !ctIn.IsNTT {
		return fmt.Errorf("cannot AutomorphismSelect: degree-1 ciphertexts in the NTT domain")
	}
	in, out, err := b.twins(ctIn, opOut)
	if err != nil {
		return err
	}
	e := b.Evaluator
	s := C.int32_t(sel)
	if err = lockedCall(func() C.int {
		return C.he_automorphism_ct_select(e.h, in[0].h, in[1].h, ks.galoisSet, &s, C.int(1), out[0].h, out[1].h)
	}, ks); err != nil {
		return err
	}
	*opOut.MetaData = *ctIn.MetaData
	return nil
}
