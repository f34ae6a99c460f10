/*
 * hering_sampler.h -- the randomness source and the three ring samplers on the device: sampling.PRNG as a handle, ring.UniformSampler
 * (ring/sampler_uniform.go:44-99; ring/ringqp/samplers.go:47-55 for a ringqp.Poly), ring.GaussianSampler (ring/sampler_gaussian.go:
 * 68-265, the float64 branch) and ring.TernarySampler with a density (ring/sampler_ternary.go:130-196, kysampling :266-336,
 * computeMatrixTernary :106-128) (libhering.so).
 *
 * Elsewhere: the Encryptor and the Decryptor (hering_encryptor.h); the KeyGenerator and the sparse ternary sampler (H != 0,
 * sampleSparse :198-263, a sequential shuffle used only for secret keys: hering_keygen.h).
 * Out of scope: the arbitrary-precision Gaussian branch (sigma > 2^53 and bound > 2^64 - 1, :100);
 * a CSPRNG on the device; a restatement of sampling.KeyedPRNG (BLAKE2Xb): a keyed source is passed in as a callback.
 *
 * The same conventions as hering.h (which this header includes): 0 on success, <0 on error (HE_E*), he_last_error() for the
 * message; outputs come last.  A sampler entry carries host data (the bytes of the source) into a polynomial, as an upload does: it
 * runs after the calling thread's queued requests, returns with its device work finished, has no replay number and cannot be
 * captured in a graph (HE_EINVAL).
 *
 * THE CONTRACT.  Every sampler of the reference reads from a sampling.PRNG, an io.Reader.  A device sampler is an exact function of
 * that byte stream: given the bytes the reference's sampler would have read, it
 *   - writes every output word as the reference writes it,
 *   - consumes exactly as many bytes as the reference consumes -- the unused tail of the last buffer the reference fetched included
 *     (1024-byte buffers for the uniform and the Gaussian sampler, N-byte buffers for the Knuth-Yao walk, N / 8 + N / 8 bytes for
 *     the density 0.5),
 *   - and leaves the source at the reference's position, so that a sequence of calls stays in step.
 * A polynomial handle of B entries is B successive Read calls, entry 0 first.
 *
 * The library may fetch ahead of what a call turns out to need; bytes fetched and not consumed stay in the he_prng handle and are
 * served first by the next call on it, so the consumed positions stay the reference's.  A call first fetches what the reference
 * would consume when nothing is rejected (the Gaussian: a sixteenth more), then doubles; at 64 times that first figure it gives up
 * with HE_EPRNG instead of fetching forever (the all-0xFF stream against a modulus below its mask is such a source).  The library's
 * own copies -- the host copies of consumed bytes, the device copies of the stream and of the sampled small values -- are zeroed
 * before their memory is released; the runtime's staging of a host-to-device copy is not the library's, and a HIP error ends the
 * call at once, without the wipe.
 *
 * Gaussian, exp and log.  normFloat64 is restated exit by exit as a default amd64 build evaluates it (no fused multiply-add, every
 * float32 operation rounded on its own): the strip test, the tail of the base strip with two logarithms per round, the wedge test in
 * float32 with one exponential.  The device's exp and log are not Go's: a draw that reaches the wedge (about 3 %) or the tail (about
 * 0.05 %) equals the reference's whenever moving exp / log by a few ulps does not change its comparison -- the same kind of contract
 * as the cosines of hering_ckks_encoder.h.  A zero mantissa word in the tail gives log(0) = -Inf and the norm +Inf, which the bound
 * rejects, as in the reference.  The tables kn / wn / fn are generated from the Marsaglia-Tsang construction with the host's libm
 * (he_gaussian_tables_host), not copied.
 *
 * Differences from the reference, deliberate:
 *   - a Knuth-Yao walk that reaches column 55 of matrixProba is an index panic in the reference; here it is HE_EINVAL;
 *   - the Gaussian bound must be at most 2^62 (coeffInt and its sign travel in one word); the reference converts any float64 below
 *     2^64;
 *   - a density outside (0, 1) is HE_EINVAL (the reference panics at 1 and converts a negative float64 to uint64 above it).
 * On any error the output polynomial is undefined and the position of the source is unchanged, except that bytes already fetched
 * stay in the handle.
 *
 * Operand identity: `pol` and `polP` must be distinct polynomials (HE_EINVAL).
 */
#ifndef HERING_SAMPLER_H
#define HERING_SAMPLER_H

#include "hering.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one more status beside those of hering.h: a randomness source failed, ran short, or never lets a call finish */
enum { HE_EPRNG = -6 };

/* The reader of a callback source: writes n bytes to dst and returns 0; any other value is a failed or short read (HE_EPRNG). */
typedef int (*he_prng_read_fn)(void *user, uint8_t *dst, size_t n);

/* The system source, getrandom(2): the analogue of crypto/rand, the reference's default. */
int he_prng_create_system(he_handle *out);
/* Any sampling.PRNG (or a deterministic stream) behind `read`; `user` is passed back unchanged and must outlive the handle.  The
 * reader is called from inside a sampler entry, with that entry's context locked: it must not call the library on that context. */
int he_prng_create_callback(he_prng_read_fn read, void *user, he_handle *out);
int he_prng_destroy(he_handle prng);
/* out[0] = the bytes consumed so far in the reference's sense; out[1] = bytes fetched ahead and not yet consumed */
int he_prng_position(he_handle prng, uint64_t out[2]);

/* UniformSampler.Read (add = 0) / ReadAndAdd (add = 1: CRed(a + b, q)) into limbs 0..level of pol, a polynomial of `ring` of any
 * batch B up to 65535.  The stream is big-endian 64-bit words, each masked with SubRing.Mask and accepted when below q_i, limb after
 * limb out of one sequence of 1024-byte buffers per Read.
 * ringP != 0: the ringqp form -- per entry a Read into pol (limbs 0..level of ring) and then a Read into polP (limbs 0..levelP of
 * ringP).  ringP = 0: levelP and polP are not read.
 * Launches: 1 when no word is rejected (2 with add: the sum is a launch of its own), whatever N, the level and the batch; a
 * rejected word costs one more launch, of one workgroup, that parses the whole call again.
 * HE_EINVAL: a level the ring lacks or more than 64 limbs; pol / polP of another context or degree, with too few limbs or with
 * unequal batches; pol == polP; inside a graph capture. */
int he_sampler_uniform_read(he_handle ring, int level, he_handle ringP, int levelP, he_handle prng, int add, he_handle pol, he_handle polP);

/* GaussianSampler.Read / ReadAndAdd with DiscreteGaussian{sigma, bound} into limbs 0..level of pol.  The stream is little-endian;
 * every draw advances 8 bytes.  The words are (c * sign) | (q_i - c) * (sign ^ 1): the word q_i itself for c = 0, sign = 0.  add:
 * CRed(a + w, q_i), wrapping in 64 bits.  montgomery: MForm of every word of limbs 0..level after that (:177-179 transform the
 * whole polynomial, the sum included).  2 launches: the parse, one workgroup; the expansion into the limbs.
 * HE_EINVAL also: sigma not in (0, 2^53]; bound negative, not finite or above 2^62. */
int he_sampler_gaussian_read(he_handle ring, int level, he_handle prng, double sigma, double bound, int montgomery, int add, he_handle pol);

/* TernarySampler.Read / ReadAndAdd with Ternary{P: p} into limbs 0..level of pol: matrixValues[i][index], the words {0, 1, q_i - 1}
 * (montgomery: {0, MForm(1), MForm(q_i - 1)}).  p = 0.5: N / 8 coefficient bytes, then N / 8 sign bytes per entry.  Any other p:
 * the Knuth-Yao walk over N-byte buffers -- the matrix of computeMatrixTernary with its float64 truncations, the bits of a byte from
 * the lowest, the restart at the same bit when d > 1, the sign from the next bit of the byte or from bit 0 of the next byte, the
 * following walk starting at that next bit (at bit 1 after a sign from the next byte).  2 launches.
 * HE_EINVAL also: p not in (0, 1); a walk that reaches column 55. */
int he_sampler_ternary_read(he_handle ring, int level, he_handle prng, double p, int montgomery, int add, he_handle pol);

/* Diagnostics: the Knuth-Yao walk over ANY pair of matrix words (bit 55 - j of x0 / x1 is column j of matrixProba[0] / [1]).  For
 * every density p with fl(1 - p) < 1 (every p above 2^-54), (1 - p) 2^56 and p 2^56 are integers that add up to 2^56 exactly, and over such a
 * pair no stream reaches the restart on d > 1 or column 55 (the walk always ends at the lowest column that holds a one); this
 * entry is how the tests reach those two branches.  A smaller p rounds 1 - p to 1: the words are 2^56 and 0, every column is empty
 * and every walk reaches column 55 (HE_EINVAL, where the reference panics). */
int he_debug_sampler_ternary_words(he_handle ring, int level, he_handle prng, uint64_t x0, uint64_t x1, int montgomery, int add, he_handle pol);

/* kn (128 words), then the float32 words of wn (128) and of fn (128), as the device holds them */
int he_gaussian_tables_host(uint32_t out[384]);
/* out[0], out[1] = the words computeMatrixTernary(1 - p) cuts matrixProba[0] and [1] from: bit 55 - j is column j */
int he_ternary_matrix_host(double p, uint64_t out[2]);

#ifdef __cplusplus
}
#endif
#endif /* HERING_SAMPLER_H */
