/*
 * hering_ckks_evaluator.h -- the coefficient-level work of the reference's ckks.Evaluator (schemes/ckks/evaluator.go) that is not
 * already one call of hering.h: Add / Sub of whole ciphertexts with a fused scale-up of one side, the scalar forms, the plaintext
 * products and MulRelinThenAdd, each as ONE launch over every component of the ciphertext (libhering.so).  Ciphertext x ciphertext
 * Mul / MulRelin (he_ckks_mul_relin), Rescale (he_div_round_by_last_modulus[_many]_ntt), Relinearize, the rotations and InnerSum
 * are the entries of hering.h, unchanged.
 *
 * The same conventions as hering.h (which this header includes): 0 on success, <0 on error (HE_E*), he_last_error() for the
 * message; outputs are caller-allocated and come last.  The caller plans levels, scales and scalar words (as with
 * hering_polyeval.h): the library takes numbers and polynomials.  Every entry is one queued request: concurrent single-ciphertext
 * callers are coalesced into one launch over entry tables, it works under deferred submission and records under
 * he_graph_begin / he_graph_end like every other operator entry.
 *
 * Operands.  All polynomials are in the NTT domain, on the limbs 0 .. level.  A component list holds 1 to 3 handles (degree 0, 1
 * or 2).  All operands share one batch, except that a plaintext of batch 1 is broadcast over the batch of the ciphertext.
 * Shapes and operand identity are checked before anything is filed: a rejected call changes no operand.
 *
 * Words.  For polynomial words below their moduli, and scalar / ratio / pre words below theirs (a word at or above its modulus
 * in s0, s1, ratio or pre is HE_EINVAL), the outputs are the words the reference's sequence of ring operations leaves: canonical
 * residues, with one exception it shares with the reference -- a component that he_ckks_add only negates holds Ring.Neg's word
 * q - x, which is q (not 0) for x = 0.  For a polynomial word at or above its modulus the output word is unspecified (no
 * reduction is applied to the inputs of an addition); no other word of the output is affected by it.
 *
 * Deliberate differences from the reference:
 *  - Scales, levels, the choice of which side is scaled and the encoding of scalar and vector operands belong to the caller
 *    (lattigo_amd / hering.hpp / go/hering plan them); the library has no rlwe.Scale.
 *  - he_ckks_mul_pt takes one component count for the ciphertext and the accumulator.  The reference's scale-up of a wider
 *    accumulator (:1087-1096 acts on every component of opOut) is he_ckks_scalar(op 2) on the further components.
 *  - he_ckks_mul_relin_then_add refuses an output that is an input with HE_EINVAL where the reference returns its error
 *    (:918, :1064).
 */
#ifndef HERING_CKKS_EVALUATOR_H
#define HERING_CKKS_EVALUATOR_H

#include "hering.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HE_CKKS_SCALAR_ADD 0
#define HE_CKKS_SCALAR_SUB 1
#define HE_CKKS_SCALAR_MUL 2
#define HE_CKKS_SCALAR_MUL_THEN_ADD 3

/* evaluateInPlace (schemes/ckks/evaluator.go:221-408) with Ring.Add (sub = 0) or Ring.Sub (sub = 1): on the common components
 * out_i = op0_i +- op1_i; the components beyond the lower degree are copied, or negated (Sub, :152-156) when they come from op1.
 * n_out = max(n0, n1).  scaled = 1 (op0) or 2 (op1): every component of that operand is first multiplied by the integer whose
 * residues are ratio[0 .. level] -- the reference's Mul(ct, ratioInt, tmp) (:259, :272, :296, :322, :352, :376), fused, with no
 * temporary; scaled = 0: ratio is not read (may be null).  Any output may be any input, crossed components included (every
 * input word of a coefficient is read before any output word of it is written); two outputs that are one polynomial are
 * HE_EINVAL.  An op1 of batch 1 is broadcast. */
int he_ckks_add(he_handle ring, int level, int sub, int n0, const he_handle *op0, int n1, const he_handle *op1, int scaled,
                const uint64_t *ratio, int n_out, const he_handle *out);

/* evaluateWithScalar (:410-424) after its preparation loop: s0[0 .. level] is the scalar for the coefficients [0, N/2) of a limb,
 * s1 for [N/2, N) -- plain residues, the pair he_double_rns_scalarop takes.  op: HE_CKKS_SCALAR_*.
 *   ADD / SUB (:80-86, :171-177): out_0 = op0_0 +- s; out_i = op0_i for i >= 1 (nothing is moved where out_i is op0_i).
 *   MUL (:629-666): out_i = op0_i * s for every component.
 *   MUL_THEN_ADD (:928-975): out_i = [pre] out_i + op0_i * s; pre (optional, null: none): out is first multiplied by the integer
 *   with the residues pre[0 .. level], the Mul(opOut, scaleInt, opOut) of :959-964.  pre with another op is HE_EINVAL.
 * n components in op0 and out.  out_i may be any op0_k. */
int he_ckks_scalar(he_handle ring, int level, int op, int n, const he_handle *op0, const uint64_t *s0, const uint64_t *s1,
                   const uint64_t *pre, const he_handle *out);

/* The plaintext branches of mulRelin (:842-869; then_add = 0) and mulRelinThenAdd (:1158-1170; then_add = 1):
 *   out_i = [[pre] out_i +] ct_i * pt,  i < n,
 * with MForm(pt) taken inside, once per coefficient, for all components.  pre (optional, then_add only): the scale-up of the
 * accumulator of :1087-1096, an integer by its residues.  pt (not in Montgomery form) may have batch 1.  out_i may be any ct_k or
 * pt. */
int he_ckks_mul_pt(he_handle ring, int level, int n, const he_handle *ct, he_handle pt, int then_add, const uint64_t *pre,
                   const he_handle *out);

/* The ciphertext x ciphertext branch of mulRelinThenAdd (:1104-1155) on degree-1 operands (a0, a1), (b0, b1) at `level`:
 *   rlk = 0:  out0 = [pre] out0 + a0 b0,  out1 = [pre] out1 + a0 b1 + a1 b0,  out2 = [pre] out2 + a1 b1   (MulThenAdd);
 *   rlk != 0: (out0, out1) = [pre] (out0, out1) + (a0 b0, a0 b1 + a1 b0) + GadgetProduct(a1 b1, rlk); out2 must be 0
 *             (MulRelinThenAdd: one tensor launch and the launches of he_relinearize).
 * pre (optional): the scale-up of the accumulator (:1087-1096).  The key's level must reach `level`.  An output that is an input,
 * and two outputs that are one polynomial, are HE_EINVAL. */
int he_ckks_mul_relin_then_add(he_handle eval, int level, he_handle a0, he_handle a1, he_handle b0, he_handle b1, he_handle rlk,
                               const uint64_t *pre, he_handle out0, he_handle out1, he_handle out2);

#ifdef __cplusplus
}
#endif
#endif /* HERING_CKKS_EVALUATOR_H */
