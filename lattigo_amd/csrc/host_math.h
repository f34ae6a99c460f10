// host_math.h -- host-side (CPU, set-up only) construction of the per-ring constants the
// kernels consume.  These are the *mathematical definitions* of the reference's tables
//  computed with plain 128-bit modular arithmetic; the
// resulting words must equal the reference's (ring/subring.go:99-159, ring/ring.go:329-346,
// ring/basis_extension.go:25-49,101-172) because NTT outputs depend on the choice of psi
// and lazy ModUp outputs on the constants.  Independent of oracle/ by construction.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "modarith.h"

namespace he {

uint64_t mulmod(uint64_t a, uint64_t b, uint64_t m);
uint64_t powmod(uint64_t a, uint64_t e, uint64_t m);
uint64_t invmod(uint64_t a, uint64_t p);  // p prime
bool is_prime_u64(uint64_t n);
std::vector<uint64_t> unique_prime_factors(uint64_t n);
uint64_t to_mont(uint64_t a, uint64_t q);  // a * 2^64 mod q

struct SubRingHost {
    ModConst mc;
    uint64_t primroot;
    std::vector<uint64_t> roots_fwd, roots_bwd;  // [N]
};
// returns false and fills err if (N, q) does not define an NTT-enabled SubRing
bool build_subring(int logN, uint64_t q, SubRingHost &out, std::string &err);
// Conjugate-invariant SubRing Z[X+X^-1]/(X^2N+1) (ring/ring.go:260, NthRoot = 4N).  The transform of
// ring/ntt.go:757-786 / :1104-1152 is a fold with roots[1] around a standard butterfly network whose stage
// with h blocks uses roots4N[2h+i]; roots_fwd/bwd are returned already remapped to that network
// (tw[h+i] = roots4N[2h+i], N entries), the fold twiddles in mc.pad0 (forward) / mc.pad1 (backward),
// and mc.ninv = MForm((2N)^-1).
bool build_subring_ci(int logN, uint64_t q, SubRingHost &out, std::string &err);

// RescaleConstants[j-1][i] = MForm(q_i - q_j^-1 mod q_i), i < j   (ring/ring.go:329-346)
std::vector<std::vector<uint64_t>> build_rescale_constants(const std::vector<uint64_t> &moduli);

// GenModUpConstants(S, D): a[i], T[j][i], vt[j][v]  (ring/basis_extension.go:101-172)
struct ModUpHost {
    int nsrc, ndst;
    std::vector<uint64_t> a, T, vt;
};
ModUpHost build_modup_constants(const std::vector<uint64_t> &S, const std::vector<uint64_t> &D);

// floor(prod(S)/2) mod m  (S all odd)
uint64_t half_product_mod(const std::vector<uint64_t> &S, uint64_t m);
// (prod(S))^-1 mod q, Montgomery form  (ring/basis_extension.go:25-49)
uint64_t inv_product_mont(const std::vector<uint64_t> &S, uint64_t q);
// multiword (little-endian) scalar mod q
uint64_t words_mod(const uint64_t *w, int n, uint64_t q);

// ---- CKKS encoder (schemes/ckks) -------------------------------------------------------------------------------------
// GetRootsComplex128(M) (schemes/ckks/utils.go:53-77): M + 1 complex128 as (re, im) pairs.  cos(angle * float64(i)) for the first
// quarter only (this host's libm), every other word a copy or a negation of those, written as :60-74 write them
void ckks_roots_complex128(uint64_t M, double *out);
// rotGroup[j] = 5^j mod M, j < M / 4 (schemes/ckks/encoder.go:83-89)
std::vector<uint32_t> ckks_rot_group(uint64_t M);
// Mixed-radix (Garner) constants of the first min(n, cap) moduli, [cap][cap]: g[i][j] = MForm(q_0 .. q_{j-1} mod q_i) for j < i,
// g[i][i] = MForm((q_0 .. q_{i-1})^-1 mod q_i); they do not depend on the level
std::vector<uint64_t> build_garner_table(const std::vector<uint64_t> &moduli, int cap);
// prod(moduli[0..n)) little-endian in `cap` words, followed by that product >> 1 in `cap` words (n <= cap)
std::vector<uint64_t> product_and_half_words(const std::vector<uint64_t> &moduli, int n, int cap);

// ---- ring samplers (ring/sampler_gaussian.go, ring/sampler_ternary.go) -------------------------------------------------------
// The ziggurat tables of normFloat64 (sampler_gaussian.go:267 on) from their construction (Marsaglia and Tsang, "The Ziggurat
// Method for Generating Random Variables", 2000: 128 strips, r = 3.442619855899, v = 9.91256303526217e-3, m1 = 2^31), doubles
// rounded once to uint32 / float32: out[0..128) = kn, out[128..256) = the words of wn, out[256..384) = the words of fn
void gaussian_ziggurat_tables(uint32_t out[384]);
// computeMatrixTernary (sampler_ternary.go:106-128): x0 = uint64(p * 2^56), x1 = uint64((1 - p) * 2^56) for p = the inverse density;
// matrixProba[r][j] = bit 55 - j of x_r, j < 55
void ternary_matrix_words(double inv_density, uint64_t &x0, uint64_t &x1);

}  // namespace he
