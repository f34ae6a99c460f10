/*
 * hering_bfv.h -- BFV: the scale-invariant multiplication of the reference's bgv.Evaluator with ScaleInvariant = true
 * (schemes/bgv/evaluator.go:898-1071: tensorScaleInvariant, modUpAndNTT, tensorLowDeg, quantize; its precomputation
 * newEvaluatorPrecomp, :38-70) (libhering.so).
 *
 * The same conventions as hering.h (which this header includes): 0 on success, <0 on error (HE_E*), he_last_error() for the
 * message; outputs are caller-allocated and come last; every product entry files its work on the context's queue (coalescing,
 * deferred submission) and records under he_graph_begin / he_graph_end like every other operator entry point.  Queued requests of
 * these entries are served one by one (their launches run over contiguous scratch and take no entry tables), as the
 * degree-changing forms of hering_ringswitch.h and hering_bridge.h are.
 *
 * Rings.  Standard rings only: a conjugate-invariant evaluator or ringQMul is HE_EINVAL (the reference's bgv parameters are
 * always standard, schemes/bgv/params.go:69).  ringQMul is Parameters.RingQMul() (params.go:98-109): a ring of the evaluator's
 * degree and context whose moduli are coprime to Q.
 *
 * Operand identity (checked before anything is filed; a rejected call changes no operand).  he_bfv_mul_relin: ANY output may be
 * ANY input -- the inputs are consumed into scratch (inverse transforms and the two tensor products) before the first output
 * word is written; two outputs that are the same polynomial are HE_EINVAL.  he_bfv_quantize: outQ may be cQ; cM is on the QMul
 * side and may be no other operand.
 */
#ifndef HERING_BFV_H
#define HERING_BFV_H

#include "hering.h"

#ifdef __cplusplus
extern "C" {
#endif

/* newEvaluatorPrecomp (evaluator.go:38-70) on the device evaluator `eval` (he_evaluator_create over RingQ, RingP): the basis
 * extender Q <-> QMul (basisExtenderQ1toQ2, the constants of he_basis_extender_create), the table
 * levelQMul[level] = ceil((bitlen(Q_level) + logN) / 61) - 1 (:43-48) and MForm(t mod q_i) per Q limb.
 * HE_EINVAL: ringQMul of another context, degree or ring type than the evaluator's; a conjugate-invariant evaluator; more than
 * 32 moduli in Q or in QMul (the cap of ModUpExact, ring/basis_extension.go:285); fewer moduli in ringQMul than
 * levelQMul[top level] + 1; t = 0.  HE_EPARAM: Q and QMul share a modulus.  The handle keeps `eval` and `ringQMul` alive. */
int he_bfv_evaluator_create(he_handle eval, he_handle ringQMul, uint64_t t, he_handle *out);
int he_bfv_evaluator_destroy(he_handle bfv);
/* levelQMul[level] of the table above */
int he_bfv_level_qmul(he_handle bfv, int level, int *level_qmul);

/* tensorScaleInvariant (evaluator.go:898-972) on degree-1 NTT-domain ciphertexts (a0, a1), (b0, b1) at `level`:
 *   modUpAndNTT (:991) of every input component into QMul at lm = levelQMul[level], tensorLowDeg (:1003) on Q and on QMul,
 *   quantize (:1050) of the three products -- the division by Q of the value held on Q x QMul, back on Q and times t -- and,
 *   with a key, the relinearisation (:966-969): (out0, out1) = (c0, c1) + GadgetProduct(c2, rlk).
 * rlk = 0: the degree-2 result (out0, out1, out2).  Otherwise the key must reach `level` (HE_EINVAL), the result is
 * (out0, out1) and out2 is ignored (pass 0), as in he_bgv_mul_relin.
 * b0 == a0 and b1 == a1 (the same handles) is the reference's squaring branch (:929, :1025): only two components are extended;
 * the words are those of the general branch.
 * Outputs are canonical.  Batched handles: every operand of B entries, B <= 16383 (one launch covers the 4B extended components). */
int he_bfv_mul_relin(he_handle bfv, int level, he_handle a0, he_handle a1, he_handle b0, he_handle b1, he_handle rlk, he_handle out0,
                     he_handle out1, he_handle out2);

/* quantize(level, levelQMul[level], c2Q1, c2Q2) (evaluator.go:1050-1071) as a piece: cQ on limbs 0..level of Q and cM on limbs
 * 0..levelQMul[level] of QMul, both in the NTT domain (any 64-bit representative: the inverse transforms reduce their input);
 * outQ = NTT(MulScalar(ModUpPtoQ(ModDownQPtoP(INTT(cQ), INTT(cM))), t)) on limbs 0..level, NTT domain, canonical.
 * Two inverse transforms, ONE launch of the fused kernel, one forward transform. */
int he_bfv_quantize(he_handle bfv, int level, he_handle cQ, he_handle cM, he_handle outQ);

#ifdef __cplusplus
}
#endif
#endif /* HERING_BFV_H */
