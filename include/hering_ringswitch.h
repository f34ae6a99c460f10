/*
 * hering_ringswitch.h -- ring-degree switching and rlwe.Evaluator.ApplyEvaluationKey (libhering.so).
 *
 * The same conventions as hering.h (which this header includes): 0 on success, <0 on error (HE_E*), he_last_error() for the
 * message; outputs are caller-allocated and come last; every entry files its work on the context's queue (coalescing, deferred
 * submission) and records under he_graph_begin / he_graph_end like every other operator entry point.
 *
 * Degrees.  A small polynomial of degree n and a large one of degree N = n * gap: both powers of two, gap >= 1, n >= 16.  A poly
 * handle does not carry its moduli: the limbs of a small polynomial are residues of the large ring's moduli, limb for limb, as in
 * the reference (core/rlwe/element.go:250-313 runs the large ring's tables on both).  Batches must match (HE_EINVAL).
 *
 * Operand identity (checked before anything is filed; a rejected call changes no operand):
 *  - handles of different degree cannot coincide;
 *  - at equal degree he_map_small_to_large_ntt(x, x), he_switch_ring_degree_ntt(r, l, x, x) and he_switch_ring_degree(l, x, x)
 *    are no-ops, and any other pair of distinct handles is a copy of limbs 0..level;
 *  - he_apply_evaluation_key at equal degree: any output may be any input, as with he_relinearize (the bootstrapping circuits
 *    call ApplyEvaluationKey(ct, evk, ct)); out0 == out1 is HE_EINVAL in every form.
 */
#ifndef HERING_RINGSWITCH_H
#define HERING_RINGSWITCH_H

#include "hering.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ring.MapSmallDimensionToLargerDimensionNTT (ring/operations.go:380): polLarge[j * gap + s] = polSmall[j] on limbs 0..level */
int he_map_small_to_large_ntt(he_handle polSmall, he_handle polLarge, int level);
/* rlwe.SwitchCiphertextRingDegreeNTT on one polynomial (core/rlwe/element.go:250): the direction is set by the two degrees;
 * ringLarge (degree max(N_in, N_out)) is required for large -> small and may be 0 otherwise; equal degrees = copy.
 * Large -> small is one pass, out[j] = gap^-1 sum_{s<gap} in[j gap + s] mod q (the reference's INTT at N, stride and NTT at n,
 * word for word for inputs in [0, 2q): canonical words and the lazy words the reference's transforms take; four lazy words sum to
 * at most 8q - 4 < 2^64 at q < 2^61.  Words at or above 2q are outside the domain); canonical output.  Limbs 0..level.
 * The batch is the launch's gridDim.z, as for the other ring-level entries of hering.h: no limit is stated and none is needed
 * (batches 65535, 65536 and 65537 are tested through the fold, the replication and both strides). */
int he_switch_ring_degree_ntt(he_handle ringLarge, int level, he_handle in, he_handle out);
/* rlwe.SwitchCiphertextRingDegree on one polynomial (core/rlwe/element.go:293), coefficient domain, limbs 0..level:
 * down out[w] = in[w gap]; up out[w gap] = in[w] and the other words of out are left untouched, as in the reference */
int he_switch_ring_degree(int level, he_handle in, he_handle out);
/* rlwe.Evaluator.ApplyEvaluationKey (core/rlwe/evaluator_evaluationkey.go:36-106), NTT-domain degree-1 ciphertexts:
 * in and out of the evaluator's degree N (same degree), in of degree n < N and out of degree N (small -> large), or in of
 * degree N and out of degree n (large -> small); the key is of degree N in every case.  HE_EINVAL when the large side is not
 * the evaluator's degree (:51-53, :68-70).  out0 = in0 + GadgetProduct(in1)_0, out1 = GadgetProduct(in1)_1 at min(level, the
 * key's level), with the degree maps of the reference before (small -> large) or after (large -> small) the key switch. */
int he_apply_evaluation_key(he_handle eval, int level, he_handle in0, he_handle in1, he_handle evk, he_handle out0, he_handle out1);

#ifdef __cplusplus
}
#endif
#endif /* HERING_RINGSWITCH_H */
