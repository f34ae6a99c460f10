package hering

/*
#include "hering_rgsw_encryptor.h"
*/
import "C"

import (
	"fmt"
	"unsafe"

	"github.com/tuneinsight/lattigo/v6/core/rlwe"
	"github.com/tuneinsight/lattigo/v6/ring"
)

// RGSWCiphertext mirrors rgsw.Ciphertext on the device: Value [2]rlwe.GadgetCiphertext as two keys of one evaluator and shape.
type RGSWCiphertext struct {
	Value [2]*EvaluationKey
}

// RGSWEncryptor mirrors rgsw.Encryptor (core/rgsw/encryptor.go; include/hering_rgsw_encryptor.h): an Encryptor whose Encrypt and
// EncryptZero take an RGSW ciphertext.  Secret-key encryption only.  Every call is an exact function of the bytes the PRNG serves;
// the drawing order is the reference's: per row (i, j) one encryptZeroSk on Value[0][i][j], then one on Value[1][i][j].
type RGSWEncryptor struct {
	*Encryptor
}

// NewRGSWEncryptor: rgsw.NewEncryptor(params, key).
func NewRGSWEncryptor(eval *Evaluator, prng *PRNG, xe ring.DiscreteGaussian, key *SecretKey) (*RGSWEncryptor, error) {
	var k interface{}
	if key != nil {
		k = key
	}
	enc, err := NewEncryptor(eval, prng, ring.Ternary{P: 2.0 / 3.0}, xe, k)
	if err != nil {
		return nil, err
	}
	return &RGSWEncryptor{Encryptor: enc}, nil
}

// NewRGSWCiphertext: rgsw.NewCiphertext, a zeroed ciphertext at the levels ResolveEvaluationKeyParameters gives.
func NewRGSWCiphertext(kgen *KeyGenerator, evkParams ...rlwe.EvaluationKeyParameters) (*RGSWCiphertext, error) {
	ct := &RGSWCiphertext{}
	for u := range ct.Value {
		k, err := kgen.NewEvaluationKey(evkParams...)
		if err != nil {
			return nil, err
		}
		ct.Value[u] = k
	}
	return ct, nil
}

// EncryptZero on an RGSW ciphertext (encryptor.go:77-121).
func (enc *RGSWEncryptor) EncryptZero(ct *RGSWCiphertext) error {
	return lockedCall(func() C.int {
		return C.he_rgsw_encrypt_zero(enc.Encryptor.h, ct.Value[0].h, ct.Value[1].h)
	}, enc, ct)
}

// Encrypt (encryptor.go:25-73): EncryptZero, then pt times the gadget vector added to component 0 of Value[0] and component 1 of
// Value[1]; pt nil: EncryptZero.
func (enc *RGSWEncryptor) Encrypt(pt *Plaintext, ct *RGSWCiphertext) error {
	if pt == nil {
		return enc.EncryptZero(ct)
	}
	return lockedCall(func() C.int {
		return C.he_rgsw_encrypt(enc.Encryptor.h, pt.Value.h, flag(pt.IsNTT), flag(pt.IsMontgomery), ct.Value[0].h, ct.Value[1].h)
	}, enc, pt, ct)
}

func rgswHandles(cts []*RGSWCiphertext) (k0, k1 []Handle) {
	k0 = make([]Handle, len(cts))
	k1 = make([]Handle, len(cts))
	for i, ct := range cts {
		k0[i], k1[i] = ct.Value[0].h, ct.Value[1].h
	}
	return
}

// EncryptTable: cts[k] = Encrypt(entry sel[k] of pts) for k = 0, 1, ... on the one source; pts holds its plaintexts as batch
// entries (NTT and Montgomery; nil when every sel is -1); sel[k] = -1 is EncryptZero.
func (enc *RGSWEncryptor) EncryptTable(pts *Poly, sel []int32, cts []*RGSWCiphertext) error {
	if len(sel) != len(cts) || len(cts) == 0 {
		return fmt.Errorf("cannot EncryptTable: %d selections for %d ciphertexts", len(sel), len(cts))
	}
	k0, k1 := rgswHandles(cts)
	return lockedCall(func() C.int {
		return C.he_rgsw_encrypt_table(enc.Encryptor.h, polyHandle(pts), (*C.int32_t)(unsafe.Pointer(&sel[0])), C.int(len(cts)), &k0[0], &k1[0])
	}, enc, pts, cts)
}

// BlindRotationKeys is what GenBlindRotationEvaluationKeyNew returns: blindrot.MemBlindRotationEvaluationKeySet over device keys.
type BlindRotationKeys struct {
	BlindRotationKeys []*RGSWCiphertext
	AutomorphismKeys  []*GaloisKey
}

// GenBlindRotationEvaluationKeyNew: blindrot.GenEvaluationKeyNew (core/rgsw/blindrot/keys.go:46-108).  enc carries skRLWE and the
// source of the RGSW ciphertexts, kgen that of the Galois keys; on one PRNG the RGSW ciphertexts draw first.  skLWE lives in ringLWE.
func GenBlindRotationEvaluationKeyNew(enc *RGSWEncryptor, kgen *KeyGenerator, ringLWE *Ring, skLWE *SecretKey, evkParams ...rlwe.EvaluationKeyParameters) (*BlindRotationKeys, error) {
	const windowSize = 10
	n := ringLWE.n
	out := &BlindRotationKeys{BlindRotationKeys: make([]*RGSWCiphertext, n), AutomorphismKeys: make([]*GaloisKey, windowSize+1)}
	for i := range out.BlindRotationKeys {
		ct, err := NewRGSWCiphertext(kgen, evkParams...)
		if err != nil {
			return nil, err
		}
		out.BlindRotationKeys[i] = ct
	}
	params := kgen.eval.params
	gks := make([]Handle, windowSize+1)
	for i := range out.AutomorphismKeys {
		evk, err := kgen.NewEvaluationKey(evkParams...)
		if err != nil {
			return nil, err
		}
		galEl := params.RingQ().NthRoot() - ring.GaloisGen
		if i < windowSize {
			galEl = params.GaloisElement(i + 1)
		}
		out.AutomorphismKeys[i] = &GaloisKey{EvaluationKey: evk, GaloisElement: galEl, NthRoot: params.RingQ().NthRoot()}
		gks[i] = evk.h
	}
	k0, k1 := rgswHandles(out.BlindRotationKeys)
	if err := lockedCall(func() C.int {
		return C.he_blindrot_gen_evaluation_key(enc.Encryptor.h, kgen.h, ringLWE.h, skLWE.Value.Q.h, C.int(n), &k0[0], &k1[0], &gks[0])
	}, enc, kgen, ringLWE, skLWE, out); err != nil {
		return nil, err
	}
	return out, nil
}
