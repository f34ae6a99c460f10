/*
 * hering_keygen.h -- rlwe.KeyGenerator (core/rlwe/keygenerator.go) on the device, over the rings of an evaluator, the samplers of
 * hering_sampler.h and a he_prng; the sparse ternary sampler (ring/sampler_ternary.go:198-263) and
 * AddPolyTimesGadgetVectorToGadgetCiphertext (core/rlwe/gadgetciphertext.go:172-241) as entries of their own (libhering.so).
 *
 * Elsewhere: rgsw.Encryptor and the blind-rotation key generator (hering_rgsw_encryptor.h: a table of RGSW ciphertexts drawn row
 * by row, with the arithmetic after the draws and the two-key gadget term fused per chunk of ciphertexts).  Out of scope: compressed
 * (seeded, degree-0) evaluation keys and sampling.KeyedPRNG; Ternary{H} as the Encryptor's own Xs.  The threshold protocols of the
 * multiparty package -- collective public, evaluation, Galois and relinearization keys, collective key switching -- are in
 * hering_multiparty.h, over this generator's handle.
 *
 * The frame of hering_encryptor.h: 0 on success, <0 on error (HE_E*), he_last_error() for the message; outputs come last.  A call
 * runs after the calling thread's queued requests, returns with its device work finished, has no replay number and is HE_EINVAL
 * inside a graph capture.  Secret keys are held as the reference holds them -- sk.Value.Q and sk.Value.P in the NTT domain and in
 * Montgomery form, batch 1, a P handle of 0 without special primes -- and every output is distinct from every key operand
 * (HE_EINVAL; tests/keygen_aliasing.py lists the pairs).
 *
 * THE CONTRACT is that of hering_sampler.h: a call is an exact function of the byte stream of the generator's source -- the
 * reference's words, the reference's consumption, the source left at the reference's position.  THE DRAWING ORDER IS PART OF IT:
 *   genSecretKeyFromSampler (:58-70)   one ternary Read at levelQ (the density sampler, or sampleSparse)
 *   genEvaluationKey (:287-330)        for row (i, j) of evk.Value, i outer and j inner: the uniform c1 (a Read on the Q limbs, then a
 *                                      Read on the P limbs, each over its own 1024-byte buffers), then the Gaussian e -- one
 *                                      encryptZeroSk per row with IsNTT = IsMontgomery = true.  (A batched he_encrypt_zero_qp over
 *                                      the rows draws step by step over the batch instead: another order.)
 *   GenGaloisKeys (:182-196)           key after key
 * On HE_EPRNG the outputs are undefined and the consumed position of the source is that of the last draw that succeeded (for a
 * source that fails at once: unchanged).
 *
 * What is fused.  he_keygen_evaluation_key draws row by row -- the uniform words go straight into the key's component-1 storage,
 * the Gaussian parse leaves its N small values in a staging buffer of [rows][N] -- and then makes, once for the whole key, whatever
 * the number of rows: the expansion of the small values into the Q and P limbs of every component-0 row, ONE transform over all
 * those rows, and ONE launch of the kernel evk_finish, which per word computes
 *     c0 = MForm(NTT(e)) - MRed(c1, skOut) [+ MRed(skIn, MForm(P 2^(j pw2))) on the Q limbs of the row's own digit]
 * and stores it canonical in place.  Launches: 2 per row and 4 after the last draw (5 when the transform takes
 * two passes, logN > 12), plus the refresh of the derived double-precision copy where the key has one, as he_evk_commit makes it.
 * A rejected uniform word costs that row the one-workgroup parse of hering_sampler.h.
 *
 * Library-owned scratch derived from a secret -- the small Gaussian values, sk^2, the permuted sk, the positions and signs of a
 * sparse key, on the host and on the device -- is zeroed before its memory is released (a HIP error ends a call without the wipe).
 */
#ifndef HERING_KEYGEN_H
#define HERING_KEYGEN_H

#include "hering_encryptor.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rlwe.NewKeyGenerator(params) over the rings of `eval`, with Xs = Ternary{P: xs_p} and Xe = DiscreteGaussian{sigma, bound} read
 * from `prng` (which must outlive the generator). */
int he_keygen_create(he_handle eval, he_handle prng, double xs_p, double xe_sigma, double xe_bound, he_handle *kgen);
int he_keygen_destroy(he_handle kgen);

/* TernarySampler.Read with Ternary{H: hw} (sampleSparse, ring/sampler_ternary.go:198-263) into limbs 0..level of pol (batch 1):
 * ceil(hw / 8) sign bytes are read first; draw i reads 4-byte big-endian words masked to bits.Len64(N - i) bits until one is below
 * N - i, takes that entry of the index list (swap-remove) and bit i & 7 of the current sign byte (0: +1, 1: -1); the remaining
 * coefficients are 0.  The words are {0, 1, q_i - 1} (montgomery: their MForm).  hw > N is N; hw <= 0 is HE_EINVAL.  The source is
 * read as the reference reads it, without buffers: ceil(hw / 8) + 4 (draws, the rejected ones included) bytes are consumed.  The
 * walk is made on the host, into one index of matrixValues per coefficient; 1 launch (the ternary expansion) writes every limb. */
int he_keygen_ternary_sparse_read(he_handle ring, int level, he_handle prng, int hw, int montgomery, he_handle pol);

/* genSecretKeyFromSampler (:58-70) with the density sampler: the ternary Read at levelQ (montgomery = false), for levelP > -1
 * ExtendBasisSmallNormAndCenter into skP, then NTT and MForm.  levelP = -1: skP is not read. */
int he_keygen_secret_key(he_handle kgen, int levelQ, int levelP, he_handle skQ, he_handle skP);
/* GenSecretKeyWithHammingWeight (:49-56): the same with the sparse sampler */
int he_keygen_secret_key_hw(he_handle kgen, int hw, int levelQ, int levelP, he_handle skQ, he_handle skP);

/* AddPolyTimesGadgetVectorToGadgetCiphertext: pt (the key's Q limbs, NTT and Montgomery, batch 1) times the gadget vector is added
 * to component 0 of evk0 and, when evk1 != 0, to component 1 of evk1 (`for u, ct := range cts`; both keys of one shape).  Row (i, j)
 * receives pt P 2^(j pw2) on the Q limbs i (levelP + 1) + k, k = 0..levelP, that exist (the break of :218); with levelP = -1 the factor
 * is 2^(j pw2) and the limb i alone.  Canonical key words give canonical key words; the keys are committed.  1 launch per key. */
int he_gadget_add_poly(he_handle pt, he_handle evk0, he_handle evk1);

/* genEvaluationKey (:287-330), uncompressed and of degree 1, into a key made by he_evk_create / he_evk_create_base2 with
 * q == p == NULL, at that key's own levels (nQk, nPk, beta, pw2 and the window counts are read from the handle; for pw2 = 0, beta
 * must be BaseRNSDecompositionVectorSize(nQk - 1, nPk - 1)).  skIn: nQk limbs; skOut = (skOutQ, skOutP): nQk and nPk limbs.  The key
 * is written in place and committed as he_evk_commit commits it.  The fused path. */
int he_keygen_evaluation_key(he_handle kgen, he_handle skInQ, he_handle skOutQ, he_handle skOutP, he_handle evk);
/* GenEvaluationKey (:261-285): skIn and skOut (sk.Value.Q alone, NTT and Montgomery) may live in rings of a smaller degree (at least
 * 16) and at other levels than the key.  Both are mapped into the generator's ring (MapSmallDimensionToLargerDimensionNTT);
 * ExtendBasisSmallNormAndCenterNTTMontgomery (core/rlwe/utils.go:250-284: INTT and IMForm of limb 0, the sign test, the expansion,
 * NTT, MForm) builds skOut.P at the key's levelP and brings skIn to the levels of skOut; then genEvaluationKey.  skOutQ must reach
 * the key's levelQ (HE_EINVAL; the reference reads stale buffer limbs there).  A composition in front of the fused entry. */
int he_keygen_evaluation_key_sk(he_handle kgen, he_handle skInQ, he_handle skOutQ, he_handle evk);
/* GenRelinearizationKey (:113-120): skIn = MulCoeffsMontgomery(sk.Q, sk.Q) at the key's levelQ, skOut = sk */
int he_keygen_relinearization_key(he_handle kgen, he_handle skQ, he_handle skP, he_handle rlk);
/* GenGaloisKey (:140-177): skOut = AutomorphismNTTWithIndex(sk, index(gal_el^-1 mod NthRoot)) on Q and P, skIn = sk.Q.  NthRoot is
 * the ring's own (2N, or 4N for a conjugate-invariant ring).  An even gal_el is HE_EINVAL. */
int he_keygen_galois_key(he_handle kgen, uint64_t gal_el, he_handle skQ, he_handle skP, he_handle gk);
/* GenGaloisKeys (:182-196): gks[0 .. n), key after key on the one source */
int he_keygen_galois_keys(he_handle kgen, int n, const uint64_t *gal_els, he_handle skQ, he_handle skP, const he_handle *gks);

#ifdef __cplusplus
}
#endif
#endif /* HERING_KEYGEN_H */
