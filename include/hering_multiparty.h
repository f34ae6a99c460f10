/*
 * hering_multiparty.h -- the threshold protocols of the reference's multiparty package on the device, over the generator of
 * hering_keygen.h (libhering.so): PublicKeyGenProtocol (multiparty/keygen_cpk.go), EvaluationKeyGenProtocol (keygen_evk.go),
 * GaloisKeyGenProtocol (keygen_gal.go), RelinearizationKeyGenProtocol (keygen_relin.go), KeySwitchProtocol (keyswitch_sk.go) and
 * PublicKeySwitchProtocol (keyswitch_pk.go) -- SampleCRP, GenShare (the two rounds of the relinearization key), AggregateShares and
 * the finalisations.  The mirrors compose PublicKeyGenProtocol.SampleCRP and KeySwitchProtocol.SampleCRP (he_sampler_uniform_read),
 * the polynomial AggregateShares (he_add), GenPublicKey (copies) and both KeySwitch finalisations (he_add, he_poly_copy) from
 * existing entries.
 *
 * Out of scope: threshold.go (Shamir), refresh.go, additive_shares.go, mpbgv/, mpckks/, sampling.KeyedPRNG (a CRS is any he_prng,
 * as everywhere), compressed shares, and the arbitrary-precision Gaussian branch that hering_sampler.h excludes.
 *
 * The frame and THE CONTRACT are those of hering_keygen.h: 0 on success, <0 on error (HE_E*), outputs last; a call runs after the
 * calling thread's queued requests, returns with its device work finished, has no replay number and is HE_EINVAL inside a graph
 * capture; every call is an exact function of the byte streams it reads -- the reference's words, the reference's consumption, every
 * source left at the reference's position; on HE_EPRNG the outputs are undefined and the source stands after its last draw that
 * succeeded.  A party's private samplers are a he_keygen handle (its evaluator, its source, its Xs and Xe); a CRS is a he_prng.
 *
 * Storage.  Gadget-shaped CRPs, shares and keys are he_evk handles made by he_evk_create / he_evk_create_base2 with q == p == NULL,
 * of the shapes hering_keygen.h takes.  A CRP occupies component 1 of every row, a degree-0 share component 0, a round-one share of
 * the relinearization key both; an entry writes the component it names and leaves the other as it was, so ONE handle may hold the
 * CRP and the (aggregated) share, which is then already the key that he_mp_evk_finalize commits.  Polynomial shares are ordinary
 * polynomial handles.  tests/multiparty_aliasing.py lists which handles may be one.
 *
 * THE DRAWING ORDERS, which are not genEvaluationKey's:
 *   sampleCRP (keygen_evk.go:64-83)    for row (i, j), i outer and j inner: one ringqp uniform ReadNew -- a Read on the Q limbs, then a
 *                                      Read on the P limbs -- and nothing in between: the uniform draws of genEvaluationKey without
 *                                      its Gaussians
 *   GenShare (keygen_evk.go:134-180)   j OUTER and i inner, the rows with j >= BaseTwoDecompositionVectorSize[i] skipped: one Gaussian
 *                                      Read per row, from the generator's source
 *   GenShareRoundOne (keygen_relin.go:116, :133-183)
 *                                      the ephemeral key's ternary Read before any row, from the same source; then j outer and i
 *                                      inner, TWO Gaussians per row: component 0's, then component 1's
 *   GenShareRoundTwo (:211-233)        i outer and j inner, one Gaussian per row
 *   PublicKeySwitchProtocol.GenShare   two sources: EncryptZero from the encryptor's own, in the order of hering_encryptor.h, then
 *                                      one Gaussian from the protocol's noise source
 *
 * The share.  Row (i, j) is MForm(NTTLazy(e)) + skIn P 2^(j pw2) on the Q limbs of the row's own digit (with the break of :161),
 * then - MRed(crp, skOut).  Every stage is canonical, so every word is what the kernel evk_finish of hering_keygen.h computes from
 * the same e with c1 := crp, and he_mp_evk_gen_share is that path with the CRP as a separate source of c1: the Gaussians go row by
 * row (in the order above) into a staging buffer of [rows][N], and then, once for the whole share, the expansion into the Q and P
 * limbs of every row, ONE transform over all rows and ONE launch of evk_finish.  Without special primes buffQ is skIn.Q itself
 * (:118-119) and the factor 2^(j pw2).
 *
 * The relinearization key.  ROUND ONE IS NOT IN MONTGOMERY FORM: buffQ = IMForm(P s) (:113), e is NTT without MForm, and
 * MulCoeffsMontgomeryThenSub(u, crp, .) takes u in Montgomery form; the kernel rkg_round_one writes both components of every row in
 * one launch: [NTT(e0) + IMForm(P s) 2^(j pw2) on the row's own digit limbs - MRed(u, crp),  NTT(e1) + MRed(s, crp)], canonical.
 * ROUND TWO IS LAZY (:217-231): MulCoeffsMontgomeryLazy leaves [0, 2q), Add is one CRed, MulCoeffsMontgomeryThenAdd one CRed; the
 * kernel rkg_round_two restates that word sequence from round1[.][0], round1[.][1], sk, u - s (formed per word) and NTT(e), so share
 * words in [q, 2q) are the reference's and go over the wire as such.  GenRelinearizationKey (:261-276) applies MForm to both
 * components (the kernel rlk_finalize).  Each round draws row by row into a staging buffer of [rows (x 2)][N] and then makes, once
 * for the whole share: the two expansions, ONE transform over all rows (and both components), ONE launch of the round's kernel.
 *
 * Launches (tests/test_gpu_multiparty.py asserts each): he_mp_crp_gadget 1 per row (a rejected uniform word costs that row the
 * one-workgroup parse of hering_sampler.h); he_mp_evk_gen_share (to which he_mp_galois_gen_share adds the automorphisms of the secret key) and
 * he_mp_rkg_round_two 1 per row and 4 after the last draw (3 without special primes); he_mp_rkg_round_one the same after the 7 of
 * the ephemeral key (the parse and the expansion of its Read, the extension, two transforms, two MForms; 4 without special primes);
 * every transform takes one launch more where it runs in two passes, logN > 12.  he_mp_gadget_aggregate and he_mp_rlk_finalize 1;
 * he_mp_evk_finalize none (copies); both finalisations refresh the derived double-precision copy where the key has one, as
 * he_evk_commit does.  The polynomial-sized shares are compositions: he_mp_pk_gen_share 9 launches (5 without special primes),
 * he_mp_cks_gen_share 6 in either branch, he_mp_pcks_gen_share those of he_encrypt_zero and 5 more (NTT) or 6.
 *
 * Library-owned scratch derived from a secret -- the small Gaussian values, the permuted secret key of a Galois share, sk_in - sk_out
 * and the noise of the key-switch shares -- is zeroed before its memory is released (a HIP error ends a call without the wipe).
 */
#ifndef HERING_MULTIPARTY_H
#define HERING_MULTIPARTY_H

#include "hering_keygen.h"

#ifdef __cplusplus
extern "C" {
#endif

/* EvaluationKeyGenProtocol.SampleCRP / GaloisKeyGenProtocol.SampleCRP (sampleCRP): the CRP matrix from the common reference string
 * `crs` into component 1 of every row of evk (a key of `eval`), at the key's own levels. */
int he_mp_crp_gadget(he_handle eval, he_handle crs, he_handle evk);

/* EvaluationKeyGenProtocol.GenShare: skIn (nQk limbs) and skOut = (skOutQ, skOutP) as he_keygen_evaluation_key takes them; crp holds
 * the CRP in component 1; the share goes to component 0 of `share`, of the shape of crp (HE_EINVAL) and possibly crp itself. */
int he_mp_evk_gen_share(he_handle kgen, he_handle skInQ, he_handle skOutQ, he_handle skOutP, he_handle crp, he_handle share);

/* GaloisKeyGenProtocol.GenShare (keygen_gal.go:48-71): skIn = sk.Q, skOut = AutomorphismNTT(sk, gal_el^-1 mod NthRoot) on Q and P,
 * NthRoot the ring's own (4N on a conjugate-invariant ring).  Refuses what he_keygen_galois_key refuses: an even gal_el, and on a
 * conjugate-invariant ring one that is not a power of 5. */
int he_mp_galois_gen_share(he_handle kgen, uint64_t gal_el, he_handle skQ, he_handle skP, he_handle crp, he_handle share);

/* AggregateShares of the gadget-shaped shares (keygen_evk.go:186-215, keygen_relin.go:237-254): out = a + b on components 0..degree
 * (degree 0 or 1) of every row, ONE Add -- a single CRed, not a full reduction -- per word, so words in [q, 2q) of lazy shares come
 * out as the reference's.  The three keys have one evaluator and shape; out may be a or b; the other components of out stay. */
int he_mp_gadget_aggregate(he_handle a, he_handle b, int degree, he_handle out);

/* GenEvaluationKey / GenGaloisKey (keygen_evk.go:218-241): component 0 of share and component 1 of crp into evk, which is then
 * committed as he_evk_commit commits it.  evk may be share, crp or both (then nothing is copied). */
int he_mp_evk_finalize(he_handle share, he_handle crp, he_handle evk);

/* RelinearizationKeyGenProtocol.GenShareRoundOne: sk = (skQ, skP); crp holds the CRP in component 1; the ephemeral key u goes to
 * (ephQ, ephP) -- as the reference leaves it: the ternary words on every limb ephQ has, of which limbs 0..levelQ and the P limbs
 * 0..levelP are then NTT and Montgomery -- and the share to both components of share1, of the shape of crp and distinct from it. */
int he_mp_rkg_round_one(he_handle kgen, he_handle skQ, he_handle skP, he_handle crp, he_handle ephQ, he_handle ephP, he_handle share1);
/* GenShareRoundTwo: round1 is the aggregated round-one share (canonical words); the share goes to component 0 of share2, of the
 * shape of round1 and distinct from it, with words in [0, 2q). */
int he_mp_rkg_round_two(he_handle kgen, he_handle ephQ, he_handle ephP, he_handle skQ, he_handle skP, he_handle round1, he_handle share2);
/* GenRelinearizationKey: rlk = [MForm(round2[.][0]), MForm(round1[.][1])], committed.  rlk may be round1 or round2. */
int he_mp_rlk_finalize(he_handle round1, he_handle round2, he_handle rlk);

/* PublicKeyGenProtocol.GenShare (keygen_cpk.go:62-75) at the parameters' top levels: share = MForm(NTT(e)) - MRed(sk, crp) on Q and
 * P.  The share is distinct from sk and crp.  skP, crpP, shareP: 0 without special primes. */
int he_mp_pk_gen_share(he_handle kgen, he_handle skQ, he_handle skP, he_handle crpQ, he_handle crpP, he_handle shareQ, he_handle shareP);

/* KeySwitchProtocol.GenShare (keyswitch_sk.go:82-118) at `level`: share = MulCoeffsMontgomeryLazy(c1, skIn - skOut) + e, with the
 * ciphertext in the NTT domain (is_ntt: the Gaussian Read, NTT, Add) or not (NTTLazy of c1, the lazy product, INTTLazy, ReadAndAdd);
 * words in [0, 2q).  e is DiscreteGaussian{sigma, bound} read from the generator's source: the mirrors pass sigma =
 * sqrt(NoiseFreshSK^2 + noise.Sigma^2) and bound = 6 sigma, as NewKeySwitchProtocol does (:49-52).  The share is distinct from the
 * three inputs. */
int he_mp_cks_gen_share(he_handle kgen, int level, he_handle skInQ, he_handle skOutQ, he_handle c1, int is_ntt, double sigma, double bound,
                        he_handle share);

/* PublicKeySwitchProtocol.GenShare (keyswitch_pk.go:69-105) at `level`: EncryptZero under the public key `enc` is bound to
 * (he_encryptor_set_key, kind 2), drawn from the encryptor's own source in the order of hering_encryptor.h and with the ciphertext's
 * (is_ntt, is_montgomery), into (share0, share1); then share0 += c1 s + e in the two branches of :93-104, with e =
 * DiscreteGaussian{sigma, bound} read from `noise_prng`.  Two sources, each left at its own position.  Deliberate difference: the
 * shares and c1 reach `level` (HE_EINVAL otherwise), where the reference encrypts at one level and adds at another.  The shares are
 * distinct from each other, from skQ and from c1. */
int he_mp_pcks_gen_share(he_handle enc, he_handle noise_prng, int level, he_handle skQ, he_handle c1, int is_ntt, int is_montgomery,
                         double sigma, double bound, he_handle share0, he_handle share1);

#ifdef __cplusplus
}
#endif
#endif /* HERING_MULTIPARTY_H */
