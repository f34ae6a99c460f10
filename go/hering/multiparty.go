package hering

/*
#include "hering_multiparty.h"
*/
import "C"

import (
	"fmt"
	"math"

	"github.com/tuneinsight/lattigo/v6/core/rlwe"
)

func minInt(a, b int) int {
	if a < b {
		return a
	}
	return b
}

// The threshold protocols of the reference's multiparty package on the device (include/hering_multiparty.h): a party's private
// samplers are its KeyGenerator, the common reference string any PRNG.  Every call is an exact function of the byte streams it reads,
// in the reference's drawing orders.  Gadget-shaped CRPs and shares live in EvaluationKey handles: a CRP in component 1, a degree-0
// share in component 0, a round-one share of the relinearization protocol in both.

// GadgetShare is a gadget-shaped share or CRP of the protocols.
type GadgetShare struct {
	*EvaluationKey
	Degree        int    // the components in use, minus one
	GaloisElement uint64 // GaloisKeyGenShare
}

// EvaluationKeyGenProtocol mirrors multiparty.EvaluationKeyGenProtocol (and, with GenGaloisShare, GaloisKeyGenProtocol).
type EvaluationKeyGenProtocol struct{ kgen *KeyGenerator }

func NewEvaluationKeyGenProtocol(kgen *KeyGenerator) EvaluationKeyGenProtocol {
	return EvaluationKeyGenProtocol{kgen: kgen}
}

// AllocateShare: a zeroed share at the resolved levels.
func (p EvaluationKeyGenProtocol) AllocateShare(evkParams ...rlwe.EvaluationKeyParameters) (*GadgetShare, error) {
	evk, err := p.kgen.NewEvaluationKey(evkParams...)
	if err != nil {
		return nil, err
	}
	return &GadgetShare{EvaluationKey: evk}, nil
}

// SampleCRP: sampleCRP, i outer and j inner, one ringqp uniform ReadNew per row.
func (p EvaluationKeyGenProtocol) SampleCRP(crs *PRNG, evkParams ...rlwe.EvaluationKeyParameters) (*GadgetShare, error) {
	crp, err := p.AllocateShare(evkParams...)
	if err != nil {
		return nil, err
	}
	return crp, lockedCall(func() C.int { return C.he_mp_crp_gadget(p.kgen.eval.h, crs.h, crp.EvaluationKey.h) }, p.kgen, crs, crp)
}

// GenShare: EvaluationKeyGenProtocol.GenShare, a share of degree 0.
func (p EvaluationKeyGenProtocol) GenShare(skIn, skOut *SecretKey, crp, shareOut *GadgetShare) error {
	shareOut.Degree = 0
	return lockedCall(func() C.int {
		return C.he_mp_evk_gen_share(p.kgen.h, skIn.Value.Q.h, skOut.Value.Q.h, polyHandle(skOut.Value.P), crp.EvaluationKey.h, shareOut.EvaluationKey.h)
	}, p.kgen, skIn, skOut, crp, shareOut)
}

// GenGaloisShare: GaloisKeyGenProtocol.GenShare.
func (p EvaluationKeyGenProtocol) GenGaloisShare(sk *SecretKey, galEl uint64, crp, shareOut *GadgetShare) error {
	if err := lockedCall(func() C.int {
		return C.he_mp_galois_gen_share(p.kgen.h, C.uint64_t(galEl), sk.Value.Q.h, polyHandle(sk.Value.P), crp.EvaluationKey.h, shareOut.EvaluationKey.h)
	}, p.kgen, sk, crp, shareOut); err != nil {
		return err
	}
	shareOut.GaloisElement, shareOut.Degree = galEl, 0
	return nil
}

// AggregateShares: share3 = share1 + share2, one Add per word on components 0..Degree.
func (p EvaluationKeyGenProtocol) AggregateShares(share1, share2, share3 *GadgetShare) error {
	if share1.GaloisElement != share2.GaloisElement {
		return fmt.Errorf("cannot aggregate: GaloisKeyGenShares do not share the same GaloisElement: %d != %d", share1.GaloisElement, share2.GaloisElement)
	}
	share3.GaloisElement = share1.GaloisElement
	return lockedCall(func() C.int {
		return C.he_mp_gadget_aggregate(share1.EvaluationKey.h, share2.EvaluationKey.h, C.int(share1.Degree), share3.EvaluationKey.h)
	}, share1, share2, share3)
}

// GenEvaluationKey: the share and the CRP into evk, committed.
func (p EvaluationKeyGenProtocol) GenEvaluationKey(share, crp *GadgetShare, evk *EvaluationKey) error {
	return lockedCall(func() C.int { return C.he_mp_evk_finalize(share.EvaluationKey.h, crp.EvaluationKey.h, evk.h) }, share, crp, evk)
}

// GenGaloisKey: GenEvaluationKey with the share's Galois element.
func (p EvaluationKeyGenProtocol) GenGaloisKey(share, crp *GadgetShare, gk *GaloisKey) error {
	if err := p.GenEvaluationKey(share, crp, gk.EvaluationKey); err != nil {
		return err
	}
	gk.GaloisElement, gk.NthRoot = share.GaloisElement, p.kgen.eval.params.RingQ().NthRoot()
	return nil
}

// RelinearizationKeyGenProtocol mirrors multiparty.RelinearizationKeyGenProtocol.
type RelinearizationKeyGenProtocol struct{ EvaluationKeyGenProtocol }

func NewRelinearizationKeyGenProtocol(kgen *KeyGenerator) RelinearizationKeyGenProtocol {
	return RelinearizationKeyGenProtocol{EvaluationKeyGenProtocol{kgen: kgen}}
}

// AllocateShare: the ephemeral key at the parameters' top levels, a degree-1 and a degree-0 share.
func (p RelinearizationKeyGenProtocol) AllocateShare(evkParams ...rlwe.EvaluationKeyParameters) (ephSk *SecretKey, r1, r2 *GadgetShare, err error) {
	ev := p.kgen.eval
	ephSk = &SecretKey{}
	if ephSk.Value.Q, err = ev.RingQ.NewPoly(1); err != nil {
		return
	}
	if ev.RingP != nil {
		if ephSk.Value.P, err = ev.RingP.NewPoly(1); err != nil {
			return
		}
	}
	if r1, err = p.EvaluationKeyGenProtocol.AllocateShare(evkParams...); err != nil {
		return
	}
	r1.Degree = 1
	r2, err = p.EvaluationKeyGenProtocol.AllocateShare(evkParams...)
	return
}

// GenShareRoundOne: the ephemeral key into ephSkOut, the degree-1 share into shareOut.
func (p RelinearizationKeyGenProtocol) GenShareRoundOne(sk *SecretKey, crp *GadgetShare, ephSkOut *SecretKey, shareOut *GadgetShare) error {
	shareOut.Degree = 1
	return lockedCall(func() C.int {
		return C.he_mp_rkg_round_one(p.kgen.h, sk.Value.Q.h, polyHandle(sk.Value.P), crp.EvaluationKey.h, ephSkOut.Value.Q.h, polyHandle(ephSkOut.Value.P),
			shareOut.EvaluationKey.h)
	}, p.kgen, sk, crp, ephSkOut, shareOut)
}

// GenShareRoundTwo: the degree-0 share, words in [0, 2q) as the reference leaves them.
func (p RelinearizationKeyGenProtocol) GenShareRoundTwo(ephSk, sk *SecretKey, round1, shareOut *GadgetShare) error {
	shareOut.Degree = 0
	return lockedCall(func() C.int {
		return C.he_mp_rkg_round_two(p.kgen.h, ephSk.Value.Q.h, polyHandle(ephSk.Value.P), sk.Value.Q.h, polyHandle(sk.Value.P), round1.EvaluationKey.h,
			shareOut.EvaluationKey.h)
	}, p.kgen, ephSk, sk, round1, shareOut)
}

// GenRelinearizationKey: MForm of round2[.][0] and of round1[.][1], committed.
func (p RelinearizationKeyGenProtocol) GenRelinearizationKey(round1, round2 *GadgetShare, evalKeyOut *EvaluationKey) error {
	return lockedCall(func() C.int {
		return C.he_mp_rlk_finalize(round1.EvaluationKey.h, round2.EvaluationKey.h, evalKeyOut.h)
	}, round1, round2, evalKeyOut)
}

// PublicKeyGenProtocol mirrors multiparty.PublicKeyGenProtocol; SampleCRP is a ringqp UniformSampler Read, AggregateShares a Ring.Add
// and GenPublicKey two copies, all of existing entries.
type PublicKeyGenProtocol struct{ kgen *KeyGenerator }

func NewPublicKeyGenProtocol(kgen *KeyGenerator) PublicKeyGenProtocol { return PublicKeyGenProtocol{kgen: kgen} }

func (p PublicKeyGenProtocol) newPolyQP() (*PolyQP, error) {
	ev := p.kgen.eval
	out := &PolyQP{}
	var err error
	if out.Q, err = ev.RingQ.NewPoly(1); err != nil {
		return nil, err
	}
	if ev.RingP != nil {
		if out.P, err = ev.RingP.NewPoly(1); err != nil {
			return nil, err
		}
	}
	return out, nil
}

// AllocateShare: a zeroed ringqp.Poly at the parameters' top levels.
func (p PublicKeyGenProtocol) AllocateShare() (*PolyQP, error) { return p.newPolyQP() }

// SampleCRP: one ringqp uniform Read from the common reference string.
func (p PublicKeyGenProtocol) SampleCRP(crs *PRNG) (*PolyQP, error) {
	crp, err := p.newPolyQP()
	if err != nil {
		return nil, err
	}
	ev := p.kgen.eval
	return crp, lockedCall(func() C.int {
		var rp, pp Handle
		lp := 0
		if ev.RingP != nil {
			rp, pp, lp = ev.RingP.h, crp.P.h, ev.RingP.level
		}
		return C.he_sampler_uniform_read(ev.RingQ.h, C.int(ev.RingQ.level), rp, C.int(lp), crs.h, C.int(0), crp.Q.h, pp)
	}, ev, crs, crp)
}

// AggregateShares: shareOut = share1 + share2 on Q and P.
func (p PublicKeyGenProtocol) AggregateShares(share1, share2, shareOut *PolyQP) error {
	ev := p.kgen.eval
	if err := ev.RingQ.Add(share1.Q, share2.Q, shareOut.Q); err != nil {
		return err
	}
	if ev.RingP != nil {
		return ev.RingP.Add(share1.P, share2.P, shareOut.P)
	}
	return nil
}

// GenPublicKey: pubkey = (roundShare, crp).
func (p PublicKeyGenProtocol) GenPublicKey(roundShare, crp *PolyQP, pubkey *PublicKey) error {
	for k, src := range []*PolyQP{roundShare, crp} {
		if err := pubkey.Value[k].Q.CopyLvl(src.Q.limbs-1, src.Q); err != nil {
			return err
		}
		if src.P != nil {
			if err := pubkey.Value[k].P.CopyLvl(src.P.limbs-1, src.P); err != nil {
				return err
			}
		}
	}
	return nil
}

// GenShare: share = MForm(NTT(e)) - MRed(sk, crp) on Q and P, at the parameters' top levels.
func (p PublicKeyGenProtocol) GenShare(sk *SecretKey, crp, shareOut *PolyQP) error {
	return lockedCall(func() C.int {
		return C.he_mp_pk_gen_share(p.kgen.h, sk.Value.Q.h, polyHandle(sk.Value.P), crp.Q.h, polyHandle(crp.P), shareOut.Q.h, polyHandle(shareOut.P))
	}, p.kgen, sk, crp, shareOut)
}

// smudging: NewKeySwitchProtocol / NewPublicKeySwitchProtocol, DiscreteGaussian{sqrt(NoiseFreshSK^2 + noise.Sigma^2), 6 sigma}
func smudging(noiseSigma, noiseFreshSK float64) (sigma, bound float64) {
	sigma = math.Sqrt(noiseFreshSK*noiseFreshSK + noiseSigma*noiseSigma)
	return sigma, 6 * sigma
}

// KeySwitchProtocol mirrors multiparty.KeySwitchProtocol; AggregateShares and KeySwitch are Ring.Add of existing entries.
type KeySwitchProtocol struct {
	kgen         *KeyGenerator
	sigma, bound float64
}

// NewKeySwitchProtocol: (kgen, noiseFlooding.Sigma, the parameters' NoiseFreshSK) -- the argument order of every mirror.
func NewKeySwitchProtocol(kgen *KeyGenerator, noiseSigma, noiseFreshSK float64) KeySwitchProtocol {
	s, b := smudging(noiseSigma, noiseFreshSK)
	return KeySwitchProtocol{kgen: kgen, sigma: s, bound: b}
}

// GenShare: share = MulCoeffsMontgomeryLazy(ct[1], skInput - skOutput) + e, in the branch of ct.IsNTT.
func (p KeySwitchProtocol) GenShare(skInput, skOutput *SecretKey, ct *Ciphertext, shareOut *Poly) error {
	level := minInt(shareOut.limbs-1, ct.Value[1].limbs-1)
	c1 := ct.Value[1]
	return lockedCall(func() C.int {
		return C.he_mp_cks_gen_share(p.kgen.h, C.int(level), skInput.Value.Q.h, skOutput.Value.Q.h, c1.h, flag(ct.IsNTT), C.double(p.sigma), C.double(p.bound),
			shareOut.h)
	}, p.kgen, skInput, skOutput, ct, shareOut)
}

// AllocateShare: a zeroed polynomial at `level`.
func (p KeySwitchProtocol) AllocateShare(level int) (*Poly, error) {
	return p.kgen.eval.RingQ.AtLevel(level).NewPoly(1)
}

// SampleCRP: a uniform polynomial at `level` from the common reference string.
func (p KeySwitchProtocol) SampleCRP(level int, crs *PRNG) (*Poly, error) {
	r := p.kgen.eval.RingQ.AtLevel(level)
	crp, err := r.NewPoly(1)
	if err != nil {
		return nil, err
	}
	var none Handle
	return crp, lockedCall(func() C.int {
		return C.he_sampler_uniform_read(r.h, C.int(level), none, C.int(0), crs.h, C.int(0), crp.h, none)
	}, r, crs, crp)
}

// AggregateShares: shareOut = share1 + share2.
func (p KeySwitchProtocol) AggregateShares(share1, share2, shareOut *Poly) error {
	if share1.limbs != share2.limbs || share1.limbs != shareOut.limbs {
		return fmt.Errorf("cannot AggregateShares: shares levels do not match")
	}
	return p.kgen.eval.RingQ.AtLevel(share1.limbs-1).Add(share1, share2, shareOut)
}

// KeySwitch: opOut = (ctIn[0] + combined, ctIn[1]).
func (p KeySwitchProtocol) KeySwitch(ctIn *Ciphertext, combined *Poly, opOut *Ciphertext) error {
	level := ctIn.Value[0].limbs - 1
	if ctIn != opOut {
		if err := opOut.Value[1].CopyLvl(level, ctIn.Value[1]); err != nil {
			return err
		}
		opOut.MetaData, opOut.Level = ctIn.MetaData, level
	}
	return p.kgen.eval.RingQ.AtLevel(level).Add(ctIn.Value[0], combined, opOut.Value[0])
}

// PublicKeySwitchProtocol mirrors multiparty.PublicKeySwitchProtocol: the party's Encryptor (its own source) and a noise source.
type PublicKeySwitchProtocol struct {
	enc          *Encryptor
	noise        *PRNG
	sigma, bound float64
}

// NewPublicKeySwitchProtocol: (enc, the noise source, noiseFlooding.Sigma, the parameters' NoiseFreshSK).
func NewPublicKeySwitchProtocol(enc *Encryptor, noise *PRNG, noiseSigma, noiseFreshSK float64) PublicKeySwitchProtocol {
	s, b := smudging(noiseSigma, noiseFreshSK)
	return PublicKeySwitchProtocol{enc: enc, noise: noise, sigma: s, bound: b}
}

// GenShare: EncryptZero under pk into the share, then share[0] += ct[1] sk + e.
func (p PublicKeySwitchProtocol) GenShare(sk *SecretKey, pk *PublicKey, ct *Ciphertext, shareOut *Ciphertext) error {
	enc, err := p.enc.WithKey(pk)
	if err != nil {
		return err
	}
	level := minInt(shareOut.Value[0].limbs-1, ct.Value[1].limbs-1)
	c1, s0, s1 := ct.Value[1], shareOut.Value[0], shareOut.Value[1]
	return lockedCall(func() C.int {
		return C.he_mp_pcks_gen_share(enc.h, p.noise.h, C.int(level), sk.Value.Q.h, c1.h, flag(ct.IsNTT), flag(ct.IsMontgomery), C.double(p.sigma),
			C.double(p.bound), s0.h, s1.h)
	}, enc, p.noise, sk, pk, ct, shareOut)
}

// AllocateShare: a zeroed element of degree 1 at levelQ.
func (p PublicKeySwitchProtocol) AllocateShare(levelQ int) (*Ciphertext, error) {
	r := p.enc.eval.RingQ.AtLevel(levelQ)
	c0, err := r.NewPoly(1)
	if err != nil {
		return nil, err
	}
	c1, err := r.NewPoly(1)
	if err != nil {
		return nil, err
	}
	return &Ciphertext{Value: []*Poly{c0, c1}, MetaData: MetaData{IsNTT: true}, Level: levelQ}, nil
}

// AggregateShares: shareOut = share1 + share2 on both components.
func (p PublicKeySwitchProtocol) AggregateShares(share1, share2, shareOut *Ciphertext) error {
	if share1.Value[0].limbs != share1.Value[1].limbs {
		return fmt.Errorf("cannot AggregateShares: the two shares are at different levelQ")
	}
	r := p.enc.eval.RingQ.AtLevel(share1.Value[0].limbs - 1)
	for k := 0; k < 2; k++ {
		if err := r.Add(share1.Value[k], share2.Value[k], shareOut.Value[k]); err != nil {
			return err
		}
	}
	return nil
}

// KeySwitch: opOut = (ctIn[0] + combined[0], combined[1]).
func (p PublicKeySwitchProtocol) KeySwitch(ctIn, combined, opOut *Ciphertext) error {
	level := ctIn.Value[0].limbs - 1
	if ctIn != opOut {
		opOut.MetaData, opOut.Level = ctIn.MetaData, level
	}
	if err := p.enc.eval.RingQ.AtLevel(level).Add(ctIn.Value[0], combined.Value[0], opOut.Value[0]); err != nil {
		return err
	}
	return opOut.Value[1].CopyLvl(level, combined.Value[1])
}
