/*
 * hering_rgsw_encryptor.h -- rgsw.Encryptor (core/rgsw/encryptor.go) and blindrot.GenEvaluationKeyNew (core/rgsw/blindrot/keys.go:46-108)
 * on the device, over an rlwe.Encryptor of hering_encryptor.h (rgsw.Encryptor embeds *rlwe.Encryptor: the handle supplies the
 * evaluator's rings, the source and Xe) and, for the Galois keys of a blind rotation, a generator of hering_keygen.h (libhering.so).
 *
 * Out of scope: public-key RGSW encryption (encryptor.go:17: "only secret-key encryption is supported"); compressed keys and
 * sampling.KeyedPRNG; the degree-0 form of encryptZeroSk; per-row draws in parallel.
 *
 * The frame of hering_encryptor.h / hering_keygen.h: 0 on success, <0 on error (HE_E*), he_last_error() for the message; outputs come
 * last.  A call runs after the calling thread's queued requests, returns with its device work finished, has no replay number and is
 * HE_EINVAL inside a graph capture.  A SECRET key must be bound to the encryptor (he_encryptor_set_key, kind 1); under a public key
 * or with no key every entry is HE_EINVAL.
 *
 * An RGSW ciphertext is passed as in hering_rgsw.h: two key handles of the encryptor's evaluator and of one shape, made by
 * he_evk_create / he_evk_create_base2 with q == p == NULL.  The levels, BaseTwoDecomposition and the window counts are read from
 * the handles; the shape must be one genEvaluationKey serves (for pw2 = 0, beta = BaseRNSDecompositionVectorSize(levelQ, levelP);
 * for pw2 != 0 one RNS digit per Q limb).  The two handles of one ciphertext, and all handles of a table, must be distinct keys.
 *
 * THE CONTRACT is that of hering_sampler.h: a call is an exact function of the byte stream of the encryptor's source.  THE DRAWING
 * ORDER IS PART OF IT and is the reference's (encryptor.go:92-118):
 *   one RGSW ciphertext   for row (i, j) of Value[.], i outer and j inner: one encryptZeroSk on Value[0][i][j], then one on
 *                         Value[1][i][j]; each draws the uniform c1 (a Read on the Q limbs, then a Read on the P limbs when
 *                         levelP >= 0), then the Gaussian e, with IsNTT = IsMontgomery = true.  Without special primes the reference
 *                         takes the *rlwe.Ciphertext branch (:96-108): the same draws with levelP = -1.
 *   a table               ciphertext after ciphertext, key 0 first
 *   a blind-rotation set  every RGSW ciphertext, then (on the generator's source) the Galois keys, key after key
 * On HE_EPRNG the outputs are undefined and the consumed position of the source is that of the last draw that succeeded.
 *
 * What is fused.  The draws are those of he_keygen_evaluation_key: per row the uniform words go straight into the row's component-1
 * storage and the Gaussian parse leaves N small values in a staging buffer.  Everything after the draws runs ONCE PER CHUNK of
 * ciphertexts, however many the chunk holds: the expansion of the small values on Q and on P into a staging slab of one
 * (levelQ + levelP + 2)-limb entry per table row, ONE transform over the slab, and ONE launch of rgsw_table_finish, which reaches
 * the separately allocated keys through a device table of their base addresses and per word of table row (k, u, i, j) computes
 *     c0 = CRed(MForm(NTT(e)) + q - MRed(c1, sk))
 * and, when sel[k] >= 0, on the Q limbs of the row's own digit adds MRed(pt[sel[k]], MForm(P 2^(j pw2))) to c0 for u = 0 and to c1 for
 * u = 1 (c0 from the c1 as drawn; AddPolyTimesGadgetVectorToGadgetCiphertext, core/rlwe/gadgetciphertext.go:172-241, with two keys).
 * The single-ciphertext entries are the table with n = 1.  Launches: 2 per row, and per chunk 4 with special primes,
 * 3 without, one more where the transform takes two passes (logN > 12), plus per key the refresh of the derived double-precision
 * copy where the key has one, as he_evk_commit makes it.  A rejected uniform word costs that row the one-workgroup parse of
 * hering_sampler.h.
 *
 * The chunk holds as many ciphertexts as fit a staging budget of 256 MiB (at least one, at most 65535 table rows);
 * HERING_RGSW_CHUNK_KEYS=<n>, read at each call, overrides it.  Chunk boundaries change neither a word nor the source's position.
 *
 * Library-owned scratch derived from a secret -- the small Gaussian values and their slab, the selection on the device, and in
 * he_blindrot_gen_evaluation_key the host and device copies of the centred LWE secret, the selection and the monomials -- is zeroed
 * before its memory is released (a HIP error ends a call without the wipe).
 *
 * Operand identity: every output key is distinct from every other output key (HE_EINVAL); keys and polynomials are handles of
 * different kinds.  tests/rgsw_encryptor_aliasing.py lists the pairs.
 *
 * Differences from the reference, deliberate:
 *  - the non-RGSW branch of EncryptZero passes a nil pointer on (encryptor.go:82) and is not mirrored: the Python and C++ classes
 *    forward operands that are no RGSW ciphertexts to the rlwe.Encryptor entries of hering_encryptor.h;
 *  - levelP >= 0 with a P handle of 0 in the bound key is HE_EINVAL;
 *  - he_blindrot_gen_evaluation_key takes an encryptor and a generator that may sit on one he_prng, where the reference gives each
 *    a source of its own: then all RGSW ciphertexts draw first and the Galois keys after them.
 */
#ifndef HERING_RGSW_ENCRYPTOR_H
#define HERING_RGSW_ENCRYPTOR_H

#include "hering_keygen.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rgsw.Encryptor.EncryptZero on an *rgsw.Ciphertext (encryptor.go:77-121) */
int he_rgsw_encrypt_zero(he_handle enc, he_handle rgsw0, he_handle rgsw1);
/* rgsw.Encryptor.Encrypt (:25-73): EncryptZero, then pt -- limbs 0..levelQ, batch 1; NTT'd when !pt_is_ntt and MForm'd when
 * !pt_is_montgomery, on limbs 0..levelQ of the ciphertext, as the reference's three branches do -- times the gadget vector added to
 * component 0 of Value[0] and component 1 of Value[1].  pt == 0: the nil plaintext (EncryptZero). */
int he_rgsw_encrypt(he_handle enc, he_handle pt, int pt_is_ntt, int pt_is_montgomery, he_handle rgsw0, he_handle rgsw1);
/* n successive Encrypt calls on the one source, ciphertext 0 first: pts holds m plaintexts (batch m, limbs 0..levelQ, NTT and
 * Montgomery; 0 when every sel is -1), sel[k] in [-1, m) picks the plaintext of ciphertext k, -1 is EncryptZero.  sel is host data
 * and is read during the call. */
int he_rgsw_encrypt_table(he_handle enc, he_handle pts, const int32_t *sel, int n, const he_handle *rgsw0, const he_handle *rgsw1);
/* blindrot.GenEvaluationKeyNew (keys.go:46-108) into n = N(ringLWE) RGSW ciphertexts and windowSize + 1 = 11 Galois keys, all of one
 * shape.  skLWE = sk.Value.Q of the LWE ring (NTT, Montgomery; limb 0 alone is read): INTT and IMForm at level 0, centred as
 * PolyToBigintCentered centres (a word >= q0 >> 1 is taken minus q0).  The distinct values s give the monomials NewMonomialXi(s)
 * (the index masked to 2N - 1, values >= N wrapped to negative, a negative i written as q - 1 at N + i), NTT'd at the ring's full
 * level and MForm'd at the keys' levelQ; the table entry runs with sel[i] = the index of s_i.  Then he_keygen_galois_keys on kgen
 * (of the encryptor's evaluator) under the encryptor's secret key for 5^1 .. 5^10 mod 2N and 2N - 5, in that order, into gks. */
int he_blindrot_gen_evaluation_key(he_handle enc, he_handle kgen, he_handle ringLWE, he_handle skLWE, int n, const he_handle *rgsw0,
                                   const he_handle *rgsw1, const he_handle *gks);

#ifdef __cplusplus
}
#endif
#endif /* HERING_RGSW_ENCRYPTOR_H */
