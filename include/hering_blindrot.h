/*
 * hering_blindrot.h -- blind rotation (core/rgsw/blindrot, libhering.so): BlindRotateCore for a batch of accumulators, each on
 * its own schedule, and the two per-entry primitives it is made of -- the RGSW external product of hering_rgsw.h and the
 * key-switched automorphism below.
 *
 * The same conventions as hering.h and hering_rgsw.h (which this header includes): 0 on success, <0 on error (HE_E*),
 * he_last_error() for the message; outputs are caller-allocated and come last; every entry files its work on the context's queue
 * and records under he_graph_begin / he_graph_end.  Host arrays (sel, a) are scalar arguments: read during the call, frozen in a
 * captured graph.
 *
 * Levels come from the keys (LevelQ(), LevelP() of the set's keys): polynomials need at least levelQ + 1 limbs and limbs above
 * levelQ keep their words.  Polynomials are in the NTT domain; input words lie in [0, 2q).
 *
 * he_automorphism_ct_select.  Batch entry b gets rlwe.Evaluator.Automorphism (core/rlwe/evaluator_automorphism.go:13-56) with
 * key sel[b] of the set and that key's Galois element; sel[b] == -1 copies the entry.  The output words are the reference's:
 * GadgetProduct (canonical), ringQ.Add of in0 with its single conditional subtraction (:43), AutomorphismNTTWithIndex (:46-47).
 * Operand identity as in the RGSW select form: out0 == in0 and / or out1 == in1 is allowed and gives the words of the
 * out-of-place call; in0 == in1 is allowed; every other pair is HE_EINVAL and changes nothing.
 * The entry is ONE launch that does the whole automorphism of a batch entry in one workgroup, after the small launches that
 * write the selection into scratch.  It exists only inside that kernel's domain and is HE_EINVAL outside it: standard rings,
 * BaseTwoDecomposition != 0, at most one special prime, and the one-launch domain of hering_rgsw.h for (logN, levelQ + 1).
 * With BaseTwoDecomposition == 0 the reference's key switch takes the centred DecomposeAndSplit
 * (evaluator_gadget_product.go:254-256): that form is served by he_automorphism_ct, not here.
 *
 * he_blind_rotate_core.  BlindRotateCore (core/rgsw/blindrot/evaluator.go:135-229, windowSize = 10) for every batch entry of the
 * accumulator, in place; a is [batch][n_lwe] words mod 2N, row b for entry b.  The schedule of a row is the reference's, word
 * for word (csrc/blindrot_plan.h lists what that includes: a[i] in {0, 1, 2N - 1} share set 0; the lookup of k = 2N finds no
 * set).  A non-zero even a[i] -- the reference panics -- is HE_EINVAL before anything is filed.  The RGSW set needs at least
 * n_lwe keys, the Galois set a key for every element the schedules use (g^1 .. g^10 and 2N - g with g = 5 cover all).
 * Routes.  Where both select forms accept the shape the batch runs in merged rounds: a round is one he_automorphism_ct_select
 * launch followed by one he_rgsw_external_product_select launch, each over the whole batch with -1 for the entries that have
 * nothing to do; launches whose selection is all -1 are skipped and there are as many rounds as the longest entry needs alone,
 * whatever the batch.  The selections of all rounds are written into scratch once per call.  Everywhere else, and with
 * HERING_NO_BLINDROT_BATCH=1 or HERING_NO_RGSW_FUSED=1 (read once), every entry runs the reference's own order through the
 * launches of he_rgsw_external_product and he_automorphism_ct: every shape those two accept, with bit-identical results.
 */
#ifndef HERING_BLINDROT_H
#define HERING_BLINDROT_H

#include "hering_rgsw.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a table of n Galois keys of one shape, key i for the Galois element gal_els[i] (odd, distinct), resident on the device with
 * the keys' automorphism index tables (BlindRotationEvaluationKeySet.GetEvaluationKeySet, blindrot/keys.go:41); the set keeps
 * its keys alive */
int he_galois_keyset_create(he_handle eval, int n, const uint64_t *gal_els, const he_handle *keys, he_handle *set);
int he_galois_keyset_destroy(he_handle set);
/* batch entry b: Automorphism with key sel[b] of the set; sel[b] == -1: out[b] = in[b] (limbs 0..levelQ).  n_sel == batch. */
int he_automorphism_ct_select(he_handle eval, he_handle in0, he_handle in1, he_handle set,
                              const int32_t *sel, int n_sel, he_handle out0, he_handle out1);
/* BlindRotateCore of every batch entry of (acc0, acc1), in place; a: [batch][n_lwe]; batch is the accumulator's */
int he_blind_rotate_core(he_handle eval, const uint64_t *a, int batch, int n_lwe, he_handle acc0, he_handle acc1,
                         he_handle rgsw_set, he_handle galois_set);

#ifdef __cplusplus
}
#endif
#endif /* HERING_BLINDROT_H */
