package hering

/*
#include "hering_keygen.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"runtime"
	"unsafe"

	"github.com/tuneinsight/lattigo/v6/core/rlwe"
	"github.com/tuneinsight/lattigo/v6/ring"
)

// KeyGenerator mirrors rlwe.KeyGenerator (core/rlwe/keygenerator.go) over the rings of an evaluator (include/hering_keygen.h).
// Every call is an exact function of the bytes the PRNG serves: the words, the drawing order (an evaluation key row after row, the
// uniform c1 and then the Gaussian e; Galois keys key after key) and the position of the source afterwards are the reference's.
type KeyGenerator struct {
	h    Handle
	eval *Evaluator
	prng *PRNG
	enc  *Encryptor
}

// GaloisKey mirrors rlwe.GaloisKey on the device.
type GaloisKey struct {
	*EvaluationKey
	GaloisElement, NthRoot uint64
}

var errCompressed = errors.New("hering: compressed evaluation keys are not on the device (include/hering_keygen.h)")

// NewKeyGenerator: rlwe.NewKeyGenerator(params) with Xs = xs (a density), Xe = xe read from prng.
func NewKeyGenerator(eval *Evaluator, prng *PRNG, xs ring.Ternary, xe ring.DiscreteGaussian) (*KeyGenerator, error) {
	enc, err := NewEncryptor(eval, prng, xs, xe, nil)
	if err != nil {
		return nil, err
	}
	k := &KeyGenerator{eval: eval, prng: prng, enc: enc}
	if err := lockedCall(func() C.int {
		return C.he_keygen_create(eval.h, prng.h, C.double(xs.P), C.double(xe.Sigma), C.double(xe.Bound), &k.h)
	}, eval, prng); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(k, func(k *KeyGenerator) { C.he_keygen_destroy(k.h) })
	return k, nil
}

// SparseTernaryRead: TernarySampler.Read with ring.Ternary{H: hw} (sampleSparse) into limbs 0..level of pol.
func SparseTernaryRead(r *Ring, prng *PRNG, hw int, montgomery bool, pol *Poly) error {
	return lockedCall(func() C.int {
		return C.he_keygen_ternary_sparse_read(r.h, C.int(r.level), prng.h, C.int(hw), flag(montgomery), pol.h)
	}, r, prng, pol)
}

func skLevelP(sk *SecretKey) int {
	if sk.Value.P == nil {
		return -1
	}
	return sk.Value.P.limbs - 1
}

// GenSecretKey: genSecretKeyFromSampler with the density sampler.
func (k *KeyGenerator) GenSecretKey(sk *SecretKey) error {
	return lockedCall(func() C.int {
		return C.he_keygen_secret_key(k.h, C.int(sk.Value.Q.limbs-1), C.int(skLevelP(sk)), sk.Value.Q.h, polyHandle(sk.Value.P))
	}, k, sk)
}

// GenSecretKeyWithHammingWeight: exactly hw non-zero coefficients.
func (k *KeyGenerator) GenSecretKeyWithHammingWeight(hw int, sk *SecretKey) error {
	return lockedCall(func() C.int {
		return C.he_keygen_secret_key_hw(k.h, C.int(hw), C.int(sk.Value.Q.limbs-1), C.int(skLevelP(sk)), sk.Value.Q.h, polyHandle(sk.Value.P))
	}, k, sk)
}

// GenPublicKey: an EncryptZero of the QP element pk.Value under sk with IsNTT = IsMontgomery = true.
func (k *KeyGenerator) GenPublicKey(sk *SecretKey, pk *PublicKey) error { return k.enc.GenPublicKey(sk, pk) }

// NewEvaluationKey: newEvaluationKey, a zeroed key of degree 1 at the levels ResolveEvaluationKeyParameters gives.
func (k *KeyGenerator) NewEvaluationKey(evkParams ...rlwe.EvaluationKeyParameters) (*EvaluationKey, error) {
	params := k.eval.params
	levelQ, levelP, pw2, compressed := rlwe.ResolveEvaluationKeyParameters(params, evkParams)
	if compressed {
		return nil, errCompressed
	}
	evk := &EvaluationKey{nQk: levelQ + 1, nPk: levelP + 1, pw2: pw2}
	var err error
	if pw2 == 0 {
		beta := params.BaseRNSDecompositionVectorSize(levelQ, levelP)
		err = lockedCall(func() C.int {
			return C.he_evk_create(k.eval.h, C.int(beta), C.int(levelQ+1), C.int(levelP+1), nil, nil, &evk.h)
		}, k.eval)
	} else {
		sizes := params.BaseTwoDecompositionVectorSize(levelQ, levelP, pw2)[:levelQ+1]
		nj := make([]C.int, len(sizes))
		for i, n := range sizes {
			nj[i] = C.int(n)
		}
		err = lockedCall(func() C.int {
			return C.he_evk_create_base2(k.eval.h, C.int(pw2), &nj[0], C.int(len(nj)), C.int(levelQ+1), C.int(levelP+1), nil, nil, &evk.h)
		}, k.eval)
	}
	if err != nil {
		return nil, err
	}
	runtime.SetFinalizer(evk, func(e *EvaluationKey) { C.he_evk_destroy(e.h) })
	return evk, nil
}

// AddPolyTimesGadgetVectorToGadgetCiphertext: pt times the gadget vector added to component u of cts[u] (one or two keys).
func AddPolyTimesGadgetVectorToGadgetCiphertext(pt *Poly, cts []*EvaluationKey) error {
	if len(cts) < 1 || len(cts) > 2 {
		return fmt.Errorf("cannot AddPolyTimesGadgetVectorToGadgetCiphertext: len(cts) should be <= 2")
	}
	var second Handle
	if len(cts) == 2 {
		second = cts[1].h
	}
	return lockedCall(func() C.int { return C.he_gadget_add_poly(pt.h, cts[0].h, second) }, pt, cts)
}

// GenEvaluationKeyRaw: genEvaluationKey on operands of the key's own ring and levels (the fused entry).
func (k *KeyGenerator) GenEvaluationKeyRaw(skIn *Poly, skOut *SecretKey, evk *EvaluationKey) error {
	return lockedCall(func() C.int {
		return C.he_keygen_evaluation_key(k.h, skIn.h, skOut.Value.Q.h, polyHandle(skOut.Value.P), evk.h)
	}, k, skIn, skOut, evk)
}

// GenEvaluationKey: the two secret keys may live in rings of a smaller degree and at other levels.
func (k *KeyGenerator) GenEvaluationKey(skInput, skOutput *SecretKey, evk *EvaluationKey) error {
	return lockedCall(func() C.int {
		return C.he_keygen_evaluation_key_sk(k.h, skInput.Value.Q.h, skOutput.Value.Q.h, evk.h)
	}, k, skInput, skOutput, evk)
}

// GenRelinearizationKey: skIn = sk^2 at the key's levelQ, skOut = sk.
func (k *KeyGenerator) GenRelinearizationKey(sk *SecretKey, rlk *EvaluationKey) error {
	return lockedCall(func() C.int {
		return C.he_keygen_relinearization_key(k.h, sk.Value.Q.h, polyHandle(sk.Value.P), rlk.h)
	}, k, sk, rlk)
}

// GenGaloisKey: the key of the automorphism X^i -> X^(i galEl).
func (k *KeyGenerator) GenGaloisKey(galEl uint64, sk *SecretKey, gk *GaloisKey) error {
	if err := lockedCall(func() C.int {
		return C.he_keygen_galois_key(k.h, C.uint64_t(galEl), sk.Value.Q.h, polyHandle(sk.Value.P), gk.EvaluationKey.h)
	}, k, sk, gk); err != nil {
		return err
	}
	gk.GaloisElement, gk.NthRoot = galEl, k.eval.params.RingQ().NthRoot()
	return nil
}

// GenGaloisKeys: key after key on the one source; a nil gks[i] is a new key at the default levels.
func (k *KeyGenerator) GenGaloisKeys(galEls []uint64, sk *SecretKey, gks []*GaloisKey) error {
	if len(galEls) != len(gks) {
		return fmt.Errorf("galEls and gks must have the same length")
	}
	if len(galEls) == 0 {
		return nil
	}
	hs := make([]Handle, len(gks))
	for i := range gks {
		if gks[i] == nil {
			evk, err := k.NewEvaluationKey()
			if err != nil {
				return err
			}
			gks[i] = &GaloisKey{EvaluationKey: evk}
		}
		hs[i] = gks[i].EvaluationKey.h
	}
	if err := lockedCall(func() C.int {
		return C.he_keygen_galois_keys(k.h, C.int(len(galEls)), (*C.uint64_t)(unsafe.Pointer(&galEls[0])), sk.Value.Q.h, polyHandle(sk.Value.P),
			(*Handle)(unsafe.Pointer(&hs[0])))
	}, k, sk, gks); err != nil {
		return err
	}
	for i, g := range galEls {
		gks[i].GaloisElement, gks[i].NthRoot = g, k.eval.params.RingQ().NthRoot()
	}
	return nil
}
