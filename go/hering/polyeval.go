package hering

/*
#include "hering_polyeval.h"
*/
import "C"

import (
	"errors"
	"math/big"
	"runtime"
	"unsafe"
)

// u64ptr is the address of the first word, or nil for an empty slice (the library answers a missing array with HE_EINVAL).
func u64ptr(v []uint64) *C.uint64_t {
	if len(v) == 0 {
		return nil
	}
	return (*C.uint64_t)(unsafe.Pointer(&v[0]))
}

// OptimalSplit: bignum.OptimalSplit (utils/bignum/polynomial.go:14) through the library's restatement.
func OptimalSplit(logDegree int) (logSplit int, err error) {
	var out C.int
	err = lockedCall(func() C.int { return C.he_polyeval_optimal_split(C.int(logDegree), &out) })
	return int(out), err
}

// SplitDegree: polynomial.SplitDegree (circuits/common/polynomial/power_basis.go:31).
func SplitDegree(n int) (a, b int, err error) {
	var ca, cb C.int
	err = lockedCall(func() C.int { return C.he_polyeval_split_degree(C.int(n), &ca, &cb) })
	return int(ca), int(cb), err
}

// PolynomialDepth: ceil(log2 degree); the reference's error where level is below it (polynomial_evaluator.go:62-65).
func PolynomialDepth(degree, level int) (depth int, err error) {
	var out C.int
	err = lockedCall(func() C.int { return C.he_polyeval_depth(C.int(degree), C.int(level), &out) })
	return int(out), err
}

// PowerInfo names one power a basis holds: X^N at a level, as a ciphertext of degree 1 or 2.
type PowerInfo struct{ N, Level, Degree int }

// PolyevalLeaf is one baby step of the library's decomposition; Present bit k: it has term k (bit 0: the constant).
type PolyevalLeaf struct {
	Degree, Level, NewDegree, CtDegree int
	Present                            uint32
}

// PolyevalStep is one primitive call of the reference's evaluators (the numbering of he_polyeval_plan).
type PolyevalStep struct{ Op, Dst, Level, Degree, A, B int }

// PolyevalPlan is the library's structure of one evaluation (csrc/polyeval_plan.h).
type PolyevalPlan struct {
	LogSplit, Depth, OutLevel int
	Leaves                    []PolyevalLeaf
	Steps                     []PolyevalStep
}

func flatPowers(powers []PowerInfo) []C.int {
	v := make([]int, 0, 3*len(powers))
	for _, p := range powers {
		v = append(v, p.N, p.Level, p.Degree)
	}
	return cInts(v)
}

func cBool(b bool) C.int {
	if b {
		return 1
	}
	return 0
}

// NewPolyevalPlan asks the library for the structure of the evaluation of a polynomial of the given degree, basis (0 monomial,
// 1 Chebyshev), parity and laziness on a basis that holds `powers`.
func NewPolyevalPlan(degree, basis int, even, odd, lazy bool, powers []PowerInfo, copyInput bool) (*PolyevalPlan, error) {
	fp := flatPowers(powers)
	var n C.size_t
	call := func(out *C.int64_t, cap C.size_t) error {
		return lockedCall(func() C.int {
			return C.he_polyeval_plan(C.int(degree), C.int(basis), cBool(even), cBool(odd), cBool(lazy), cBool(copyInput),
				C.int(len(powers)), &fp[0], out, cap, &n)
		})
	}
	if err := call(nil, 0); err != nil {
		return nil, err
	}
	w := make([]int64, int(n)+1)
	if err := call((*C.int64_t)(unsafe.Pointer(&w[0])), n); err != nil {
		return nil, err
	}
	p := &PolyevalPlan{LogSplit: int(w[0]), Depth: int(w[1]), OutLevel: int(w[4])}
	at := 5
	for i := 0; i < int(w[2]); i, at = i+1, at+5 {
		p.Leaves = append(p.Leaves, PolyevalLeaf{int(w[at]), int(w[at+1]), int(w[at+2]), int(w[at+3]), uint32(w[at+4])})
	}
	for i := 0; i < int(w[3]); i, at = i+1, at+6 {
		p.Steps = append(p.Steps, PolyevalStep{int(w[at]), int(w[at+1]), int(w[at+2]), int(w[at+3]), int(w[at+4]), int(w[at+5])})
	}
	return p, nil
}

// BGVTermWords: the words of c for MulThenAdd(X, c, out) at (X.Scale, out.Scale) mod t (schemes/bgv/evaluator.go:1108-1140): the
// scale ratio, centred, reduced modulo every q_i up to level.
func BGVTermWords(Q []uint64, t uint64, level int, c, xScale, outScale uint64) []uint64 {
	T := new(big.Int).SetUint64(t)
	v := new(big.Int).SetUint64(c % t)
	if xScale != outScale {
		r := new(big.Int).ModInverse(new(big.Int).SetUint64(xScale), T)
		r.Mul(r, new(big.Int).SetUint64(outScale))
		v.Mul(v, r).Mod(v, T)
	}
	return bgvCentredWords(Q, T, level, v, nil)
}

// BGVConstWords: the words of c for Add(out, c) at out.Scale (schemes/bgv/evaluator.go:144-172): centred, times T^-1 mod Q_level.
func BGVConstWords(Q []uint64, t uint64, level int, c, outScale uint64) []uint64 {
	T := new(big.Int).SetUint64(t)
	v := new(big.Int).Mul(new(big.Int).SetUint64(c%t), new(big.Int).SetUint64(outScale%t))
	v.Mod(v, T)
	Ql := big.NewInt(1)
	for i := 0; i <= level; i++ {
		Ql.Mul(Ql, new(big.Int).SetUint64(Q[i]))
	}
	return bgvCentredWords(Q, T, level, v, new(big.Int).ModInverse(T, Ql))
}

func bgvCentredWords(Q []uint64, T *big.Int, level int, v, times *big.Int) []uint64 {
	half := new(big.Int).Rsh(T, 1)
	if v.Cmp(half) > 0 {
		v.Sub(v, T)
	}
	if times != nil {
		v.Mul(v, times)
	}
	out := make([]uint64, level+1)
	for i := range out {
		qi := new(big.Int).SetUint64(Q[i])
		out[i] = new(big.Int).Mod(v, qi).Uint64()
	}
	return out
}

// PlannedPolynomial is a polynomial planned for one basis with its scalar words resident (he_polyeval_poly_create).
type PlannedPolynomial struct {
	h    Handle
	ring *Ring
}

// NewPlannedPolynomial uploads the caller's words: per baby step in the library's order and per coefficient k = 0 .. degree,
// 1 + level(X^1) residues in s0 (coefficients [0, N/2) of a limb) and s1 ([N/2, N)); BGV passes the same words twice.
func (r *Ring) NewPlannedPolynomial(degree, basis int, even, odd, lazy bool, powers []PowerInfo, leafDegree, leafLevel []int,
	s0, s1 []uint64) (*PlannedPolynomial, error) {
	if len(powers) == 0 || len(leafDegree) == 0 || len(leafDegree) != len(leafLevel) || len(s0) == 0 || len(s0) != len(s1) {
		return nil, errors.New("NewPlannedPolynomial: powers, baby steps (one level each) and two word lists of one length are needed")
	}
	fp, ld, ll := flatPowers(powers), cInts(leafDegree), cInts(leafLevel) // (cInts never returns an empty slice)
	p := &PlannedPolynomial{ring: r}
	if err := lockedCall(func() C.int {
		return C.he_polyeval_poly_create(r.h, C.int(degree), C.int(basis), cBool(even), cBool(odd), cBool(lazy), C.int(len(powers)), &fp[0],
			C.int(len(leafDegree)), &ld[0], &ll[0], u64ptr(s0), u64ptr(s1), &p.h)
	}); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(p, func(p *PlannedPolynomial) { C.he_polyeval_poly_destroy(p.h) })
	return p, nil
}

// CheckLeaves holds the caller's baby steps against the library's decomposition without a ring.
func CheckLeaves(degree, basis int, even, odd, lazy bool, powers []PowerInfo, leafDegree, leafLevel []int) error {
	fp, ld, ll := flatPowers(powers), cInts(leafDegree), cInts(leafLevel)
	return lockedCall(func() C.int {
		return C.he_polyeval_check_leaves(C.int(degree), C.int(basis), cBool(even), cBool(odd), cBool(lazy), C.int(len(powers)), &fp[0],
			C.int(len(leafDegree)), &ld[0], &ll[0])
	})
}

// SetGroup: baby steps per launch of the leaf-group kernel, 0 (the library's default), 1, 2 or 4.
func (p *PlannedPolynomial) SetGroup(G int) error {
	return lockedCall(func() C.int { return C.he_polyeval_poly_set_group(p.h, C.int(G)) })
}

// EvaluatePolynomialFromPowerBasis: EvaluatePolynomialVectorFromPowerBasis (polynomial_evaluator.go:254) for the baby steps
// [first, first+len(out)): X[k-1] = the components of X^k (nil where the basis lacks it), out[g] = those of baby step first+g.
func (p *PlannedPolynomial) EvaluatePolynomialFromPowerBasis(first int, X [][]*Poly, out [][]*Poly) error {
	xs, os := make([]Handle, 3*len(X)+1), make([]Handle, 3*len(out)+1)
	for k, ct := range X {
		for c := 0; c < len(ct) && c < 3; c++ {
			xs[3*k+c] = h(ct[c])
		}
	}
	for g, ct := range out {
		for c := 0; c < len(ct) && c < 3; c++ {
			os[3*g+c] = h(ct[c])
		}
	}
	return lockedCall(func() C.int {
		return C.he_polyeval_leaves(p.h, C.int(first), C.int(len(out)), C.int(len(X)), &xs[0], &os[0])
	}, X, out)
}

// ChebyshevWords are the caller's numbers for the Chebyshev steps of a plan, in its order (hering_polyeval.h): Kind 0 = Add(x, -1),
// 1 / 2 = Sub with the second / first operand times the integer ratio first, 3 = Sub as it is; Words residues per entry.
type ChebyshevWords struct {
	Kind   []int
	S0, S1 []uint64
	Words  int
}

// DevicePowerBasis is polynomial.PowerBasis on the device: NewPowerBasis copies the ciphertext (c0, c1) at level into X^1.
type DevicePowerBasis struct{ h Handle }

func (e *Evaluator) NewDevicePowerBasis(basis, level int, c0, c1 *Poly) (*DevicePowerBasis, error) {
	pb := &DevicePowerBasis{}
	if err := lockedCall(func() C.int {
		return C.he_polyeval_basis_create(e.h, C.int(basis), C.int(level), h(c0), h(c1), &pb.h)
	}, c0, c1); err != nil {
		return nil, err
	}
	runtime.SetFinalizer(pb, func(pb *DevicePowerBasis) { C.he_polyeval_basis_destroy(pb.h) })
	return pb, nil
}

// Powers lists the powers the basis holds.
func (pb *DevicePowerBasis) Powers() (out []PowerInfo, err error) {
	var n C.size_t
	if err = lockedCall(func() C.int { return C.he_polyeval_basis_powers(pb.h, nil, 0, &n) }); err != nil {
		return
	}
	w := make([]C.int, 3*int(n)+3)
	if err = lockedCall(func() C.int { return C.he_polyeval_basis_powers(pb.h, &w[0], n, &n) }); err != nil {
		return
	}
	for i := 0; i < int(n); i++ {
		out = append(out, PowerInfo{int(w[3*i]), int(w[3*i+1]), int(w[3*i+2])})
	}
	return
}

func rlkHandle(rlk *EvaluationKey) Handle {
	if rlk == nil {
		return 0
	}
	return rlk.h
}

// GenPower: PowerBasis.GenPower (power_basis.go:76); scheme 0 CKKS, 1 BGV with plaintext modulus t.
func (pb *DevicePowerBasis) GenPower(scheme int, t uint64, rlk *EvaluationKey, n int, lazy bool, cw ChebyshevWords) error {
	k := cInts(cw.Kind)
	return lockedCall(func() C.int {
		return C.he_polyeval_gen_power(pb.h, C.int(scheme), C.uint64_t(t), rlkHandle(rlk), C.int(n), cBool(lazy), C.int(len(cw.Kind)), &k[0],
			u64ptr(cw.S0), u64ptr(cw.S1), C.int(cw.Words))
	}, rlk)
}

// Evaluate: polynomial.Evaluator.Evaluate (polynomial_evaluator.go:33) as ONE native call; (c0, c1) at level is left untouched.
func (p *PlannedPolynomial) Evaluate(e *Evaluator, scheme int, t uint64, rlk *EvaluationKey, level int, c0, c1 *Poly, cw ChebyshevWords,
	out0, out1 *Poly) error {
	k := cInts(cw.Kind)
	return lockedCall(func() C.int {
		return C.he_polyeval_evaluate(e.h, p.h, C.int(scheme), C.uint64_t(t), rlkHandle(rlk), C.int(level), h(c0), h(c1), C.int(len(cw.Kind)), &k[0],
			u64ptr(cw.S0), u64ptr(cw.S1), C.int(cw.Words), h(out0), h(out1))
	}, rlk, c0, c1, out0, out1)
}

// EvaluateFromPowerBasis: polynomial.Evaluator.EvaluateFromPowerBasis (:47) as ONE native call on the basis p was planned for.
func (p *PlannedPolynomial) EvaluateFromPowerBasis(pb *DevicePowerBasis, scheme int, t uint64, rlk *EvaluationKey, cw ChebyshevWords,
	out0, out1 *Poly) error {
	k := cInts(cw.Kind)
	return lockedCall(func() C.int {
		return C.he_polyeval_evaluate_from_power_basis(pb.h, p.h, C.int(scheme), C.uint64_t(t), rlkHandle(rlk), C.int(len(cw.Kind)), &k[0],
			u64ptr(cw.S0), u64ptr(cw.S1), C.int(cw.Words), h(out0), h(out1))
	}, rlk, out0, out1)
}
