/*
 * hering_encryptor.h -- rlwe.Encryptor (core/rlwe/encryptor.go) and rlwe.Decryptor (core/rlwe/decryptor.go) on the device, over the
 * rings of an evaluator, the samplers of hering_sampler.h and a he_prng (libhering.so).
 *
 * Elsewhere: the KeyGenerator beyond GenPublicKey (hering_keygen.h: genEvaluationKey is a loop of EncryptZero calls plus the gadget
 * term, with the arithmetic after the draws fused).  Out of scope: the degree-0 form of encryptZeroSk that sends c1 to scratch
 * (encryptor.go:355-359); the sparse ternary distribution as the encryptor's own Xs and whatever else hering_sampler.h leaves out.
 *
 * The same conventions as hering.h: 0 on success, <0 on error, he_last_error() for the message; outputs come last.  Like the
 * encoders and the samplers, these entries carry host data (the bytes of the source): a call runs after the calling thread's queued
 * requests, returns with its device work finished, has no replay number and is HE_EINVAL inside a graph capture.  Decrypt carries
 * no host data but keeps the same frame, so that the pair behaves alike.
 *
 * Every entry composes the public entries of hering.h and hering_sampler.h -- nothing is fused -- so its words are theirs.  THE
 * DRAWING ORDER IS PART OF THE CONTRACT (with the contract of hering_sampler.h, a call is an exact function of the byte stream):
 *   encryptZeroSk (:347-433)      uniform c1 (Q; for a QP element Q then P), then the Gaussian e into c0
 *   encryptZeroPk (:204-299)      ternary u, Gaussian e0, Gaussian e1
 *   encryptZeroPkNoP (:301-342)   ternary u, Gaussian e0 (Read + NTT + Add when IsNTT, INTT + ReadAndAdd otherwise), Gaussian e1
 * A polynomial handle of B entries is B ciphertexts.  Each draw above is then one sampler call over the B entries, entry 0 first:
 * the stream serves step by step, not ciphertext by ciphertext (B separate calls of batch 1 read the same bytes in another order).
 * Keys carry the batch of the outputs: entry b of the key encrypts entry b.
 *
 * Keys are held as the reference holds them: sk.Value and pk.Value[0 .. 1] in the NTT domain and in Montgomery form, a QP element as
 * a (Q handle, P handle) pair; without special primes (an evaluator created with ringP = 0) the P handles are 0.  The encryptor keeps
 * the handles it is given, not copies: they must outlive it or be replaced with another set_key call (WithKey is a cheap re-bind).
 *
 * Launches (hering.h's launches, counted by he_prof_begin / he_prof_end; independent of N, the level and the batch): see DESIGN.md
 * 8.6 for the table per entry.
 *
 * Operand identity: every output must be distinct from every other output, from the plaintext and from every key polynomial
 * (HE_EINVAL); tests/encryptor_aliasing.py lists the pairs.  In he_decryptor_decrypt the plaintext must be distinct from every
 * ciphertext component and from the key.
 */
#ifndef HERING_ENCRYPTOR_H
#define HERING_ENCRYPTOR_H

#include "hering_sampler.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rlwe.NewEncryptor(params, nil) over the rings of `eval`, with Xs = Ternary{P: xs_p} and Xe = DiscreteGaussian{sigma, bound} read
 * from `prng` (which must outlive the encryptor).  The reference's defaults are xs_p = 2/3, sigma = 3.2, bound = 19.2. */
int he_encryptor_create(he_handle eval, he_handle prng, double xs_p, double xe_sigma, double xe_bound, he_handle *enc);
int he_encryptor_destroy(he_handle enc);
/* Encryptor.WithKey.  kind 1: a secret key (key[0] = sk.Value.Q, key[1] = sk.Value.P); kind 2: a public key (key[0], key[1] =
 * pk.Value[0].Q, .P; key[2], key[3] = pk.Value[1].Q, .P); kind 0: no key.  A P handle may be 0: without special primes it is not
 * read; with them, a call that reads the P part of the key (the QP form under sk, every form under pk) is then HE_EINVAL, and the
 * ring.Poly form under sk, which reads sk.Value.Q only, is served. */
int he_encryptor_set_key(he_handle enc, int kind, const he_handle key[4]);

/* EncryptZero on an Element[ring.Poly] of degree 1 at `level` with the metadata (is_ntt, is_montgomery): sk -> encryptZeroSk; pk ->
 * encryptZeroPk (levelP = 0, as the reference) or, without special primes, encryptZeroPkNoP. */
int he_encrypt_zero(he_handle enc, int level, int is_ntt, int is_montgomery, he_handle c0, he_handle c1);
/* EncryptZero on an Element[ringqp.Poly] of degree 1 at (levelQ, levelP): sk -> :369-389, pk -> the :286-295 branch of encryptZeroPk.
 * GenPublicKey (keygenerator.go:80-88) is this call under sk at the top levels with is_ntt = is_montgomery = 1.  levelP = -1 under
 * sk: a ringqp.Poly without a P part (no special primes); c0P and c1P are not read. */
int he_encrypt_zero_qp(he_handle enc, int levelQ, int levelP, int is_ntt, int is_montgomery, he_handle c0Q, he_handle c0P, he_handle c1Q,
                       he_handle c1P);
/* addPtToCt (:481-507): c0 += pt on limbs 0..level, after the NTT of pt when (pt_is_ntt, !ct_is_ntt) and the INTT of pt when
 * (!pt_is_ntt, ct_is_ntt) -- as the reference writes them. */
int he_add_pt_to_ct(he_handle enc, int level, int pt_is_ntt, int ct_is_ntt, he_handle pt, he_handle c0);
/* Encrypt (:134-152): the ciphertext takes the plaintext's metadata (is_ntt, is_montgomery); level = min(pt_level, ct_level), written
 * to *level_out when not null; EncryptZero at that level, then addPtToCt. */
int he_encrypt(he_handle enc, int pt_level, int ct_level, int is_ntt, int is_montgomery, he_handle pt, he_handle c0, he_handle c1,
               int *level_out);

/* rlwe.NewDecryptor(params, sk) over ringQ of `eval`: skQ = sk.Value.Q (NTT, Montgomery), kept as a handle. */
int he_decryptor_create(he_handle eval, he_handle skQ, he_handle *dec);
int he_decryptor_destroy(he_handle dec);
/* Decryptor.Decrypt (:51-93) of ct[0 .. degree] into pt: level = min(ct_level, pt_level) (to *level_out when not null); the Horner
 * loop with its Reduce at i & 7 == 7 and after the loop when degree & 7 != 7; for is_ntt = 0 the NTTLazy of every component and the
 * final INTT.  degree in [0, 63].
 * Difference from the reference, deliberate: for is_ntt = 0 and degree & 7 == 7 the reference makes no Reduce before its INTT, which
 * then reads sums of NTTLazy words (ring/ntt.go:64: up to 6q - 2 each) on which its butterflies are not exact, so that its words
 * are not the decryption there.  Here the Reduce is made in that case too (he_ntt_lazy keeps [0, 2q), he_intt takes canonical
 * words) and pt is the canonical decryption.  Every other case is the reference's word for word. */
int he_decryptor_decrypt(he_handle dec, int ct_level, int pt_level, int is_ntt, int degree, const he_handle *ct, he_handle pt, int *level_out);

#ifdef __cplusplus
}
#endif
#endif /* HERING_ENCRYPTOR_H */
