package hering

/*
#include "hering_bgv_encoder.h"
*/
import "C"

import (
	"fmt"
	"runtime"
	"unsafe"

	"github.com/tuneinsight/lattigo/v6/core/rlwe"
	"github.com/tuneinsight/lattigo/v6/schemes/bgv"
)

// BGVEncoder mirrors bgv.Encoder (schemes/bgv/encoder.go), the encoder of BGV and BFV, on the device: Encode, Embed, EmbedScale,
// Decode, EncodeRingT, DecodeRingT, RingT2Q and RingQ2T are native calls (include/hering_bgv_encoder.h).  Values are []uint64 or
// []int64, as the reference's IntegerSlice.  The coefficient encoding (IsBatched = false) is served only when the plaintext ring
// has the degree of the ciphertext ring; the header lists the other deliberate differences.
type BGVEncoder struct {
	h      Handle
	params bgv.Parameters
	ringQ  *Ring
	ringP  *Ring // nil without special primes
	ringT  *Ring
}

// NewBGVEncoder: bgv.NewEncoder(params) (encoder.go:49) over the device twins of params.RingQ(), params.RingP() and params.RingT().
func NewBGVEncoder(ctx *Context, params bgv.Parameters) (*BGVEncoder, error) {
	rq, err := NewRing(ctx, params.RingQ())
	if err != nil {
		return nil, err
	}
	rt, err := NewRing(ctx, params.RingT())
	if err != nil {
		return nil, err
	}
	e := &BGVEncoder{params: params, ringQ: rq, ringT: rt}
	var hp Handle
	if params.RingP() != nil {
		if e.ringP, err = NewRing(ctx, params.RingP()); err != nil {
			return nil, err
		}
		hp = e.ringP.h
	}
	if err = lockedCall(func() C.int { return C.he_bgv_encoder_create(rq.h, hp, rt.h, &e.h) }); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(e, func(e *BGVEncoder) { C.he_bgv_encoder_destroy(e.h) })
	return e, nil
}

// RingT: the device twin of params.RingT(), for the polynomials of EncodeRingT / DecodeRingT / RingT2Q / RingQ2T.
func (e *BGVEncoder) RingT() *Ring { return e.ringT }

// Info: logN_T, log2 gap, the limb cap of RingQ2T / Decode, 0.
func (e *BGVEncoder) Info() (info [4]int, err error) {
	out := make([]C.int, 4)
	if err = lockedCall(func() C.int { return C.he_bgv_encoder_info(e.h, &out[0]) }); err != nil {
		return
	}
	for i := range info {
		info[i] = int(out[i])
	}
	return
}

// IndexMatrix: permuteMatrix(LogMaxSlots) (encoder.go:110) as the device holds it.
func (e *BGVEncoder) IndexMatrix() ([]uint64, error) {
	out := make([]uint64, e.params.MaxSlots())
	err := lockedCall(func() C.int { return C.he_bgv_encoder_index(e.h, (*C.uint64_t)(unsafe.Pointer(&out[0]))) }, out)
	return out, err
}

// integers: the pointer, length and signedness of a []uint64 or []int64
func integers(values interface{}) (*C.uint64_t, int, bool, error) {
	switch v := values.(type) {
	case []uint64:
		if len(v) == 0 {
			return nil, 0, false, fmt.Errorf("no values")
		}
		return (*C.uint64_t)(unsafe.Pointer(&v[0])), len(v), false, nil
	case []int64:
		if len(v) == 0 {
			return nil, 0, true, fmt.Errorf("no values")
		}
		return (*C.uint64_t)(unsafe.Pointer(&v[0])), len(v), true, nil
	}
	return nil, 0, false, fmt.Errorf("values.(type) must be either []uint64 or []int64 but is %T", values)
}

// EncodeRingT: Encoder.EncodeRingT (encoder.go:203) into pT, a device polynomial of RingT().
func (e *BGVEncoder) EncodeRingT(values interface{}, scale rlwe.Scale, pT *Poly) error {
	p, n, signed, err := integers(values)
	if err != nil {
		return fmt.Errorf("cannot EncodeRingT: %w", err)
	}
	return lockedCall(func() C.int {
		return C.he_bgv_encode_ring_t(e.h, C.uint64_t(scale.Uint64()), p, C.size_t(n), b2i(signed), C.int(1), pT.h)
	}, values)
}

// DecodeRingT: Encoder.DecodeRingT (encoder.go:341) of pT into values, []uint64 or []int64 of at least MaxSlots entries.
func (e *BGVEncoder) DecodeRingT(pT *Poly, scale rlwe.Scale, values interface{}) error {
	p, have, signed, err := integers(values)
	if err != nil {
		return fmt.Errorf("cannot DecodeRingT: %w", err)
	}
	if have < e.params.MaxSlots() {
		return fmt.Errorf("cannot DecodeRingT: len(values)=%d < %d", have, e.params.MaxSlots())
	}
	return lockedCall(func() C.int { return C.he_bgv_decode_ring_t(e.h, C.uint64_t(scale.Uint64()), pT.h, b2i(signed), p) }, values)
}

// RingT2Q: Encoder.RingT2Q (encoder.go:378) into pQ, a device polynomial of ringQ.
func (e *BGVEncoder) RingT2Q(level int, scaleUp bool, pT, pQ *Poly) error {
	return lockedCall(func() C.int { return C.he_bgv_ring_t2q(e.h, C.int(level), b2i(scaleUp), C.int(0), pT.h, pQ.h) })
}

// RingQ2T: Encoder.RingQ2T (encoder.go:412).
func (e *BGVEncoder) RingQ2T(level int, scaleDown bool, pQ, pT *Poly) error {
	return lockedCall(func() C.int { return C.he_bgv_ring_q2t(e.h, C.int(level), b2i(scaleDown), pQ.h, pT.h) })
}

// EmbedScale: Encoder.EmbedScale (encoder.go:268) into the device polynomial polyQ at its own level, and, with polyP non-nil, into
// the P half of a ringqp.Poly from the same transform modulo T.
func (e *BGVEncoder) EmbedScale(values interface{}, scaleUp bool, metadata *rlwe.MetaData, polyQ, polyP *Poly) error {
	p, n, signed, err := integers(values)
	if err != nil {
		return fmt.Errorf("cannot embed: %w", err)
	}
	levelP, hp := -1, Handle(0)
	if polyP != nil {
		levelP, hp = polyP.limbs-1, polyP.h
	}
	return lockedCall(func() C.int {
		return C.he_bgv_encode_qp(e.h, C.int(polyQ.limbs-1), C.int(levelP), C.uint64_t(metadata.Scale.Uint64()), b2i(metadata.IsNTT),
			b2i(metadata.IsMontgomery), b2i(scaleUp), p, C.size_t(n), b2i(signed), C.int(1), polyQ.h, hp)
	}, values)
}

// Embed: Encoder.Embed (encoder.go:336): EmbedScale without the factor T^-1.
func (e *BGVEncoder) Embed(values interface{}, metadata *rlwe.MetaData, polyQ, polyP *Poly) error {
	return e.EmbedScale(values, false, metadata, polyQ, polyP)
}

// Encode: Encoder.Encode (encoder.go:143).  The plaintext's value is encoded on its device twin `pt` (one batch entry, the
// plaintext's level); Download brings it to the host.
func (e *BGVEncoder) Encode(values interface{}, plaintext *rlwe.Plaintext, pt *Poly) error {
	p, n, signed, err := integers(values)
	if err != nil {
		return fmt.Errorf("cannot Encode: %w", err)
	}
	return lockedCall(func() C.int {
		return C.he_bgv_encode(e.h, C.int(plaintext.Level()), C.uint64_t(plaintext.Scale.Uint64()), b2i(plaintext.IsBatched), b2i(plaintext.IsNTT),
			b2i(plaintext.IsMontgomery), C.int(1), p, C.size_t(n), b2i(signed), C.int(1), pt.h)
	}, values)
}

// Decode: Encoder.Decode (encoder.go:470) of the device twin `pt` of plaintext into []uint64 or []int64 of at least MaxSlots
// entries.
func (e *BGVEncoder) Decode(plaintext *rlwe.Plaintext, pt *Poly, values interface{}) error {
	p, have, signed, err := integers(values)
	if err != nil {
		return fmt.Errorf("cannot Decode: %w", err)
	}
	if have < e.params.MaxSlots() {
		return fmt.Errorf("cannot Decode: len(values)=%d < %d", have, e.params.MaxSlots())
	}
	return lockedCall(func() C.int {
		return C.he_bgv_decode(e.h, C.int(plaintext.Level()), C.uint64_t(plaintext.Scale.Uint64()), b2i(plaintext.IsBatched), b2i(plaintext.IsNTT),
			pt.h, b2i(signed), p)
	}, values)
}
