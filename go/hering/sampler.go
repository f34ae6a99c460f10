package hering

/*
#include <stdlib.h>
#include "hering_sampler.h"

// (a file with an exported function may only declare in its preamble)
extern int heringPRNGRead(void *user, uint8_t *dst, size_t n);
*/
import "C"

import (
	"errors"
	"runtime"
	"runtime/cgo"
	"unsafe"

	"github.com/tuneinsight/lattigo/v6/ring"
	"github.com/tuneinsight/lattigo/v6/utils/sampling"
)

// PRNG is a sampling.PRNG behind a library handle (include/hering_sampler.h).  The device samplers are exact functions of the bytes
// the source serves: the words they write, the bytes they consume and the position they leave the source at are those of the
// reference's samplers on the same sampling.PRNG.  The library may fetch ahead; Position counts the bytes consumed.
type PRNG struct {
	h    Handle
	user cgo.Handle    // of the sampling.PRNG; zero for the system source
	cell *C.uintptr_t  // C memory holding `user`: what the library passes back to heringPRNGRead
}

var errSparseTernary = errors.New("hering: only ring.Ternary{P} is sampled on the device (Ternary{H} is the KeyGenerator's)")

//export heringPRNGRead
func heringPRNGRead(user unsafe.Pointer, dst *C.uint8_t, n C.size_t) C.int {
	src := cgo.Handle(*(*C.uintptr_t)(user)).Value().(sampling.PRNG)
	buf := unsafe.Slice((*byte)(unsafe.Pointer(dst)), int(n))
	if m, err := src.Read(buf); err != nil || m != int(n) {
		return 1
	}
	return 0
}

// NewPRNG: the system source, getrandom(2), the analogue of sampling.NewPRNG's crypto/rand.
func NewPRNG() (*PRNG, error) {
	p := &PRNG{}
	if err := lockedCall(func() C.int { return C.he_prng_create_system(&p.h) }); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(p, func(p *PRNG) { C.he_prng_destroy(p.h) })
	return p, nil
}

// NewPRNGFrom wraps any sampling.PRNG, a sampling.KeyedPRNG included: the device samplers then draw what the reference's would.
func NewPRNGFrom(src sampling.PRNG) (*PRNG, error) {
	p := &PRNG{user: cgo.NewHandle(src), cell: (*C.uintptr_t)(C.malloc(C.size_t(unsafe.Sizeof(C.uintptr_t(0)))))}
	*p.cell = C.uintptr_t(p.user)
	release := func(p *PRNG) { C.free(unsafe.Pointer(p.cell)); p.user.Delete() }
	if err := lockedCall(func() C.int {
		return C.he_prng_create_callback((C.he_prng_read_fn)(C.heringPRNGRead), unsafe.Pointer(p.cell), &p.h)
	}); err != nil {
		release(p)
		return nil, err
	}
	runtime.SetFinalizer(p, func(p *PRNG) { C.he_prng_destroy(p.h); release(p) })
	return p, nil
}

// Position: the bytes consumed so far in the reference's sense.
func (p *PRNG) Position() (uint64, error) {
	out := make([]C.uint64_t, 2)
	err := lockedCall(func() C.int { return C.he_prng_position(p.h, (*C.uint64_t)(unsafe.Pointer(&out[0]))) }, p)
	return uint64(out[0]), err
}

func flag(b bool) C.int {
	if b {
		return 1
	}
	return 0
}

// UniformSampler mirrors ring.UniformSampler (ring/sampler_uniform.go); with ringP, ringqp.UniformSampler.
type UniformSampler struct {
	prng         *PRNG
	ringQ, ringP *Ring
}

// NewUniformSampler: ring.NewUniformSampler(prng, baseRing).
func NewUniformSampler(prng *PRNG, baseRing *Ring) *UniformSampler {
	return &UniformSampler{prng: prng, ringQ: baseRing}
}

// NewUniformSamplerQP: ringqp.NewUniformSampler(prng, ringqp.Ring{RingQ, RingP}).
func NewUniformSamplerQP(prng *PRNG, ringQ, ringP *Ring) *UniformSampler {
	return &UniformSampler{prng: prng, ringQ: ringQ, ringP: ringP}
}

// AtLevel: the sampler at the given level (levelP is not read without ringP).
func (u *UniformSampler) AtLevel(levelQ, levelP int) *UniformSampler {
	c := &UniformSampler{prng: u.prng, ringQ: u.ringQ.AtLevel(levelQ)}
	if u.ringP != nil {
		c.ringP = u.ringP.AtLevel(levelP)
	}
	return c
}

func (u *UniformSampler) read(add bool, q, p *Poly) error {
	if u.ringP == nil {
		var none Handle
		return lockedCall(func() C.int {
			return C.he_sampler_uniform_read(u.ringQ.h, C.int(u.ringQ.level), none, C.int(0), u.prng.h, flag(add), q.h, none)
		}, u, q)
	}
	return lockedCall(func() C.int {
		return C.he_sampler_uniform_read(u.ringQ.h, C.int(u.ringQ.level), u.ringP.h, C.int(u.ringP.level), u.prng.h, flag(add), q.h, p.h)
	}, u, q, p)
}

// Read, ReadAndAdd: ring.UniformSampler.Read / ReadAndAdd; a batch of B entries is B successive Reads.
func (u *UniformSampler) Read(pol *Poly) error       { return u.read(false, pol, nil) }
func (u *UniformSampler) ReadAndAdd(pol *Poly) error { return u.read(true, pol, nil) }

// ReadQP, ReadAndAddQP: ringqp.UniformSampler.Read on the pair (Q, P): per entry a Read on Q, then a Read on P.
func (u *UniformSampler) ReadQP(q, p *Poly) error       { return u.read(false, q, p) }
func (u *UniformSampler) ReadAndAddQP(q, p *Poly) error { return u.read(true, q, p) }

// GaussianSampler mirrors ring.GaussianSampler (ring/sampler_gaussian.go), the float64 branch.
type GaussianSampler struct {
	prng       *PRNG
	baseRing   *Ring
	xe         ring.DiscreteGaussian
	montgomery bool
}

// NewGaussianSampler: ring.NewGaussianSampler(prng, baseRing, X, montgomery).
func NewGaussianSampler(prng *PRNG, baseRing *Ring, X ring.DiscreteGaussian, montgomery bool) *GaussianSampler {
	return &GaussianSampler{prng: prng, baseRing: baseRing, xe: X, montgomery: montgomery}
}

func (g *GaussianSampler) AtLevel(level int) *GaussianSampler {
	return &GaussianSampler{prng: g.prng, baseRing: g.baseRing.AtLevel(level), xe: g.xe, montgomery: g.montgomery}
}

func (g *GaussianSampler) read(add bool, pol *Poly) error {
	return lockedCall(func() C.int {
		return C.he_sampler_gaussian_read(g.baseRing.h, C.int(g.baseRing.level), g.prng.h, C.double(g.xe.Sigma), C.double(g.xe.Bound),
			flag(g.montgomery), flag(add), pol.h)
	}, g, pol)
}

func (g *GaussianSampler) Read(pol *Poly) error       { return g.read(false, pol) }
func (g *GaussianSampler) ReadAndAdd(pol *Poly) error { return g.read(true, pol) }

// TernarySampler mirrors ring.TernarySampler (ring/sampler_ternary.go) for ring.Ternary{P}; Ternary{H} is not on the device.
type TernarySampler struct {
	prng       *PRNG
	baseRing   *Ring
	xs         ring.Ternary
	montgomery bool
}

// NewTernarySampler: ring.NewTernarySampler(prng, baseRing, X, montgomery).
func NewTernarySampler(prng *PRNG, baseRing *Ring, X ring.Ternary, montgomery bool) (*TernarySampler, error) {
	if X.H != 0 || X.P == 0 {
		return nil, errSparseTernary
	}
	return &TernarySampler{prng: prng, baseRing: baseRing, xs: X, montgomery: montgomery}, nil
}

func (t *TernarySampler) AtLevel(level int) *TernarySampler {
	return &TernarySampler{prng: t.prng, baseRing: t.baseRing.AtLevel(level), xs: t.xs, montgomery: t.montgomery}
}

func (t *TernarySampler) read(add bool, pol *Poly) error {
	return lockedCall(func() C.int {
		return C.he_sampler_ternary_read(t.baseRing.h, C.int(t.baseRing.level), t.prng.h, C.double(t.xs.P), flag(t.montgomery), flag(add), pol.h)
	}, t, pol)
}

func (t *TernarySampler) Read(pol *Poly) error       { return t.read(false, pol) }
func (t *TernarySampler) ReadAndAdd(pol *Poly) error { return t.read(true, pol) }
