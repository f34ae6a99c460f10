package hering

/*
#include "hering_encryptor.h"
*/
import "C"

import (
	"errors"
	"runtime"
	"unsafe"

	"github.com/tuneinsight/lattigo/v6/ring"
)

// PolyQP is a ringqp.Poly on the device: a (Q, P) pair; P is nil without special primes.
type PolyQP struct{ Q, P *Poly }

// SecretKey mirrors rlwe.SecretKey on the device: Value in the NTT domain and Montgomery form.  Keys carry the batch of the
// ciphertexts they serve.
type SecretKey struct{ Value PolyQP }

// PublicKey mirrors rlwe.PublicKey on the device.
type PublicKey struct{ Value [2]PolyQP }

// MetaData: the fields of rlwe.MetaData the encryptor and the decryptor read.
type MetaData struct{ IsNTT, IsMontgomery bool }

// Plaintext and Ciphertext mirror rlwe.Plaintext / rlwe.Ciphertext over device polynomials; Level is the limbs in use minus one.
type Plaintext struct {
	Value *Poly
	MetaData
	Level int
}
type Ciphertext struct {
	Value []*Poly
	MetaData
	Level int
}

// ElementQP mirrors rlwe.Element[ringqp.Poly] of degree 1.
type ElementQP struct {
	Value [2]PolyQP
	MetaData
	LevelQ, LevelP int
}

// Encryptor mirrors rlwe.Encryptor (core/rlwe/encryptor.go) over the rings of an evaluator (include/hering_encryptor.h).  Every call
// is an exact function of the bytes the PRNG serves: the words, the drawing order and the position of the source afterwards are
// the reference's; for a batch the draws are made step by step over the entries.
type Encryptor struct {
	h    Handle
	eval *Evaluator
	prng *PRNG
	xs   ring.Ternary
	xe   ring.DiscreteGaussian
	key  interface{} // what keeps the bound key alive
}

var errNoKey = errors.New("hering: invalid key type, want *SecretKey, *PublicKey or nil")

// NewEncryptor: rlwe.NewEncryptor(params, key) with Xs = xs, Xe = xe read from prng.
func NewEncryptor(eval *Evaluator, prng *PRNG, xs ring.Ternary, xe ring.DiscreteGaussian, key interface{}) (*Encryptor, error) {
	if xs.H != 0 || xs.P == 0 {
		return nil, errSparseTernary
	}
	e := &Encryptor{eval: eval, prng: prng, xs: xs, xe: xe}
	if err := lockedCall(func() C.int {
		return C.he_encryptor_create(eval.h, prng.h, C.double(xs.P), C.double(xe.Sigma), C.double(xe.Bound), &e.h)
	}, eval, prng); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(e, func(e *Encryptor) { C.he_encryptor_destroy(e.h) })
	if err := e.bind(key); err != nil {
		return nil, err
	}
	return e, nil
}

func polyHandle(p *Poly) Handle {
	var none Handle
	if p == nil {
		return none
	}
	return p.h
}

func (e *Encryptor) bind(key interface{}) error {
	k := make([]Handle, 4)
	kind := 0
	switch key := key.(type) {
	case nil:
	case *SecretKey:
		kind, k[0], k[1] = 1, polyHandle(key.Value.Q), polyHandle(key.Value.P)
	case *PublicKey:
		kind = 2
		k[0], k[1], k[2], k[3] = polyHandle(key.Value[0].Q), polyHandle(key.Value[0].P), polyHandle(key.Value[1].Q), polyHandle(key.Value[1].P)
	default:
		return errNoKey
	}
	if err := lockedCall(func() C.int {
		return C.he_encryptor_set_key(e.h, C.int(kind), (*Handle)(unsafe.Pointer(&k[0])))
	}, e); err != nil {
		return err
	}
	e.key = key
	return nil
}

// WithKey: a shallow copy bound to key (sharing the evaluator's tables and the source).
func (e *Encryptor) WithKey(key interface{}) (*Encryptor, error) {
	if key == nil {
		key = e.key
	}
	return NewEncryptor(e.eval, e.prng, e.xs, e.xe, key)
}

// EncryptZero on an Element[ring.Poly] of degree 1, according to ct's metadata and level.
func (e *Encryptor) EncryptZero(ct *Ciphertext) error {
	return lockedCall(func() C.int {
		return C.he_encrypt_zero(e.h, C.int(ct.Level), flag(ct.IsNTT), flag(ct.IsMontgomery), ct.Value[0].h, ct.Value[1].h)
	}, e, ct)
}

// EncryptZeroQP: EncryptZero on an Element[ringqp.Poly] of degree 1.
func (e *Encryptor) EncryptZeroQP(ct *ElementQP) error {
	levelP := ct.LevelP
	if ct.Value[0].P == nil {
		levelP = -1
	}
	return lockedCall(func() C.int {
		return C.he_encrypt_zero_qp(e.h, C.int(ct.LevelQ), C.int(levelP), flag(ct.IsNTT), flag(ct.IsMontgomery), ct.Value[0].Q.h,
			polyHandle(ct.Value[0].P), ct.Value[1].Q.h, polyHandle(ct.Value[1].P))
	}, e, ct)
}

// Encrypt: the ciphertext takes the plaintext's metadata and level = min of the two; pt == nil is EncryptZero.
func (e *Encryptor) Encrypt(pt *Plaintext, ct *Ciphertext) error {
	if pt == nil {
		return e.EncryptZero(ct)
	}
	var level C.int
	if err := lockedCall(func() C.int {
		return C.he_encrypt(e.h, C.int(pt.Level), C.int(ct.Level), flag(pt.IsNTT), flag(pt.IsMontgomery), pt.Value.h, ct.Value[0].h, ct.Value[1].h, &level)
	}, e, pt, ct); err != nil {
		return err
	}
	ct.MetaData, ct.Level = pt.MetaData, int(level)
	return nil
}

// AddPtToCt: addPtToCt (encryptor.go:481-507).
func (e *Encryptor) AddPtToCt(level int, pt *Plaintext, ct *Ciphertext) error {
	return lockedCall(func() C.int {
		return C.he_add_pt_to_ct(e.h, C.int(level), flag(pt.IsNTT), flag(ct.IsNTT), pt.Value.h, ct.Value[0].h)
	}, e, pt, ct)
}

// GenPublicKey: KeyGenerator.GenPublicKey (keygenerator.go:80-88), an EncryptZero of the QP element pk.Value under sk with
// IsNTT = IsMontgomery = true.
func (e *Encryptor) GenPublicKey(sk *SecretKey, pk *PublicKey) error {
	enc, err := e.WithKey(sk)
	if err != nil {
		return err
	}
	el := &ElementQP{Value: pk.Value, MetaData: MetaData{IsNTT: true, IsMontgomery: true}, LevelQ: e.eval.RingQ.level}
	if e.eval.RingP != nil {
		el.LevelP = e.eval.RingP.level
	}
	return enc.EncryptZeroQP(el)
}

// Decryptor mirrors rlwe.Decryptor (core/rlwe/decryptor.go).
type Decryptor struct {
	h  Handle
	sk *SecretKey
}

// NewDecryptor: rlwe.NewDecryptor(params, sk).
func NewDecryptor(eval *Evaluator, sk *SecretKey) (*Decryptor, error) {
	d := &Decryptor{sk: sk}
	if err := lockedCall(func() C.int { return C.he_decryptor_create(eval.h, sk.Value.Q.h, &d.h) }, eval, sk); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(d, func(d *Decryptor) { C.he_decryptor_destroy(d.h) })
	return d, nil
}

// Decrypt: pt takes the ciphertext's metadata and level = min of the two.
func (d *Decryptor) Decrypt(ct *Ciphertext, pt *Plaintext) error {
	hs := make([]Handle, len(ct.Value))
	for i, p := range ct.Value {
		hs[i] = p.h
	}
	var level C.int
	if err := lockedCall(func() C.int {
		return C.he_decryptor_decrypt(d.h, C.int(ct.Level), C.int(pt.Level), flag(ct.IsNTT), C.int(len(ct.Value)-1), (*Handle)(unsafe.Pointer(&hs[0])), pt.Value.h, &level)
	}, d, ct, pt); err != nil {
		return err
	}
	pt.MetaData, pt.Level = ct.MetaData, int(level)
	return nil
}
