package hering

/*
#include "hering_ckks_encoder.h"
*/
import "C"

import (
	"fmt"
	"runtime"
	"unsafe"

	"github.com/tuneinsight/lattigo/v6/core/rlwe"
	"github.com/tuneinsight/lattigo/v6/ring"
	"github.com/tuneinsight/lattigo/v6/schemes/ckks"
)

// Encoder mirrors the double-precision path of ckks.Encoder (schemes/ckks/encoder.go, prec <= 53) on the device: Encode, Embed,
// Decode, DecodePublic, FFT and IFFT are native calls (include/hering_ckks_encoder.h).  The table of roots the device holds is
// ckks.GetRootsComplex128 of THIS process, so the words are Go's math.Cos bits, not those of the library's own libm.
// Values are []complex128 or []float64; the big.Float / bignum.Complex slices of the reference's arbitrary-precision path are
// not served.
type Encoder struct {
	h      Handle
	params ckks.Parameters
	ringQ  *Ring
	ringP  *Ring // nil without special primes
}

func f64ptr(v []float64) *C.double { return (*C.double)(unsafe.Pointer(&v[0])) }

func c128ptr(v []complex128) *C.double { return (*C.double)(unsafe.Pointer(&v[0])) }

// NewEncoder: ckks.NewEncoder(params) (encoder.go:78) over the device twins of params.RingQ() and params.RingP().
func NewEncoder(ctx *Context, params ckks.Parameters) (*Encoder, error) {
	rq, err := NewRing(ctx, params.RingQ())
	if err != nil {
		return nil, err
	}
	e := &Encoder{params: params, ringQ: rq}
	var hp Handle
	if params.RingP() != nil {
		if e.ringP, err = NewRing(ctx, params.RingP()); err != nil {
			return nil, err
		}
		hp = e.ringP.h
	}
	roots := ckks.GetRootsComplex128(int(params.RingQ().NthRoot()))
	if err = lockedCall(func() C.int { return C.he_ckks_encoder_create(rq.h, hp, c128ptr(roots), &e.h) }, roots); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(e, func(e *Encoder) { C.he_ckks_encoder_destroy(e.h) })
	return e, nil
}

// RootsHost: the library's own GetRootsComplex128 (its libm's cosines), for comparison with ckks.GetRootsComplex128.
func RootsHost(nthRoot int) ([]complex128, error) {
	out := make([]complex128, nthRoot+1)
	err := lockedCall(func() C.int { return C.he_ckks_roots_host(C.uint64_t(nthRoot), c128ptr(out)) }, out)
	return out, err
}

// Roots: the table the device holds.
func (e *Encoder) Roots() ([]complex128, error) {
	out := make([]complex128, int(e.params.RingQ().NthRoot())+1)
	err := lockedCall(func() C.int { return C.he_ckks_encoder_roots(e.h, c128ptr(out)) }, out)
	return out, err
}

// Info: log2 NthRoot, LogMaxDimensions.Cols, the largest logN of the one-workgroup transform, the limb cap of Decode.
func (e *Encoder) Info() (info [4]int, err error) {
	out := make([]C.int, 4)
	if err = lockedCall(func() C.int { return C.he_ckks_encoder_info(e.h, &out[0]) }); err != nil {
		return
	}
	for i := range info {
		info[i] = int(out[i])
	}
	return
}

// FFT: Encoder.FFT (encoder.go:794) on []complex128, in place.
func (e *Encoder) FFT(values []complex128, logN int) error {
	if len(values) < 1<<logN {
		return fmt.Errorf("cannot FFT: len(values)=%d < %d", len(values), 1<<logN)
	}
	return lockedCall(func() C.int { return C.he_ckks_fft(e.h, C.int(logN), C.int(1), c128ptr(values)) }, values)
}

// IFFT: Encoder.IFFT (encoder.go:765) on []complex128, in place.
func (e *Encoder) IFFT(values []complex128, logN int) error {
	if len(values) < 1<<logN {
		return fmt.Errorf("cannot IFFT: len(values)=%d < %d", len(values), 1<<logN)
	}
	return lockedCall(func() C.int { return C.he_ckks_ifft(e.h, C.int(logN), C.int(1), c128ptr(values)) }, values)
}

func b2i(b bool) C.int {
	if b {
		return 1
	}
	return 0
}

// floats: the pointer, length and complexity of a []complex128 or []float64
func floats(values interface{}) (*C.double, int, bool, error) {
	switch v := values.(type) {
	case []complex128:
		if len(v) == 0 {
			return nil, 0, true, fmt.Errorf("no values")
		}
		return c128ptr(v), len(v), true, nil
	case []float64:
		if len(v) == 0 {
			return nil, 0, false, fmt.Errorf("no values")
		}
		return f64ptr(v), len(v), false, nil
	}
	return nil, 0, false, fmt.Errorf("values.(type) must be []complex128 or []float64 (the double-precision path), but is %T", values)
}

// Embed: Encoder.Embed (encoder.go:208) into the device polynomial polyOut (a ring.Poly twin at its own level).
func (e *Encoder) Embed(values interface{}, metadata *rlwe.MetaData, polyOut *Poly) error {
	p, n, cplx, err := floats(values)
	if err != nil {
		return fmt.Errorf("cannot Embed: %w", err)
	}
	return lockedCall(func() C.int {
		return C.he_ckks_encode(e.h, C.int(polyOut.limbs-1), C.int(metadata.LogDimensions.Cols), C.double(metadata.Scale.Float64()), C.int(1),
			b2i(metadata.IsNTT), b2i(metadata.IsMontgomery), p, C.size_t(n), b2i(cplx), C.int(1), polyOut.h)
	}, values)
}

// EmbedQP: the ringqp.Poly arm of Embed (encoder.go:321-328): one IFFT feeding polyQ and polyP (nil: P.Level() = -1).
func (e *Encoder) EmbedQP(values interface{}, metadata *rlwe.MetaData, polyQ, polyP *Poly) error {
	p, n, cplx, err := floats(values)
	if err != nil {
		return fmt.Errorf("cannot Embed: %w", err)
	}
	levelP, hp := -1, Handle(0)
	if polyP != nil {
		levelP, hp = polyP.limbs-1, polyP.h
	}
	return lockedCall(func() C.int {
		return C.he_ckks_encode_qp(e.h, C.int(polyQ.limbs-1), C.int(levelP), C.int(metadata.LogDimensions.Cols), C.double(metadata.Scale.Float64()),
			b2i(metadata.IsNTT), b2i(metadata.IsMontgomery), p, C.size_t(n), b2i(cplx), C.int(1), polyQ.h, hp)
	}, values)
}

// Encode: Encoder.Encode (encoder.go:156).  The plaintext's value is encoded on its device twin `pt` (one batch entry, the
// plaintext's level); Download brings it to the host.
func (e *Encoder) Encode(values interface{}, plaintext *rlwe.Plaintext, pt *Poly) error {
	if plaintext.IsBatched {
		return e.Embed(values, plaintext.MetaData, pt)
	}
	v, ok := values.([]float64)
	if !ok || len(v) == 0 {
		return fmt.Errorf("cannot Encode: supported values.(type) for IsBatched=False is []float64, but %T was given", values)
	}
	return lockedCall(func() C.int {
		return C.he_ckks_encode(e.h, C.int(plaintext.Level()), C.int(0), C.double(plaintext.Scale.Float64()), C.int(0), b2i(plaintext.IsNTT),
			C.int(0), f64ptr(v), C.size_t(len(v)), C.int(0), C.int(1), pt.h)
	}, v)
}

// DecodePublic: Encoder.DecodePublic (encoder.go:199) of the device twin `pt` of plaintext into []complex128 or []float64 of
// at least slots (N when not batched) entries.
func (e *Encoder) DecodePublic(plaintext *rlwe.Plaintext, pt *Poly, values interface{}, logprec float64) error {
	n := 1 << plaintext.LogDimensions.Cols
	if !plaintext.IsBatched {
		n = e.params.N()
	}
	p, have, cplx, err := floats(values)
	if err != nil {
		return fmt.Errorf("cannot Decode: %w", err)
	}
	if have < n {
		return fmt.Errorf("cannot Decode: len(values)=%d < %d", have, n)
	}
	return lockedCall(func() C.int {
		return C.he_ckks_decode(e.h, C.int(plaintext.Level()), C.int(plaintext.LogDimensions.Cols), C.double(plaintext.Scale.Float64()),
			b2i(plaintext.IsBatched), b2i(plaintext.IsNTT), C.double(logprec), pt.h, b2i(cplx), p)
	}, values)
}

// Decode: Encoder.Decode (encoder.go:192).
func (e *Encoder) Decode(plaintext *rlwe.Plaintext, pt *Poly, values interface{}) error {
	return e.DecodePublic(plaintext, pt, values, 0)
}

// RingType of the encoder's parameters.
func (e *Encoder) RingType() ring.Type { return e.params.RingType() }
