/*
 * hering_ringpack.h -- the ring-packing evaluator of core/rlwe/ring_packing.go (libhering.so): Split, Merge and the inner steps of
 * Expand and Pack, from which the host mirrors build Extract[Naive] and Repack[Naive].
 *
 * The same conventions as hering.h (which this header includes): 0 on success, <0 on error (HE_E*), he_last_error() for the
 * message; outputs are caller-allocated and come last; every entry files its work on the context's queue (coalescing, deferred
 * submission) and records under he_graph_begin / he_graph_end like every other operator entry point.
 *
 * Standard rings only: on a conjugate-invariant ring every entry returns HE_EINVAL (X^(2^i) does not exist in Z[X + X^-1]; the
 * reference refuses Expand / Pack there, :491-493, :633-635).  All polynomials are in the NTT domain with canonical words (in
 * [0, q)), and every output is canonical.  Degrees: N is the ring's / evaluator's degree; Split and Merge pair it with N/2 >= 16.
 * A poly handle does not carry its moduli: the limbs of a polynomial of degree N/2 are residues of the large ring's moduli.
 * One call covers at most 65535 entries (batch entries times the two components of a ciphertext, pairs times two): a larger
 * one is HE_EINVAL, to be split by the caller.
 *
 * No monomial table exists on the device.  The reference's XPow2NTT[i] / XInvPow2NTT[i] (GenXPow2NTT, :772-810) are views of the
 * resident twiddle tables: word j is w = Roots[(N >> (i+1)) + (j >> (i+1))] where bit i of j is clear and q - w where it is set,
 * with RootsForward for X^(2^i) and RootsBackward for X^(-2^i).  he_ring_xpow2_ntt materialises one for the naive paths.
 *
 * Operand identity (checked before anything is filed; a rejected call changes no operand):
 *  - two outputs never coincide, and inputs may coincide with inputs;
 *  - an output may be an input only as out_k == in_k in the sum_only form of he_ringpack_expand_step (the reference's
 *    Add(c0, tmp, c0), :557-558); the pack steps work in place on their a / b operands by definition;
 *  - a handle that occurs twice among the a0 / a1 / b0 / b1 / t0 / t1 operands of a pack step is HE_EINVAL.
 */
#ifndef HERING_RINGPACK_H
#define HERING_RINGPACK_H

#include "hering.h"

#ifdef __cplusplus
extern "C" {
#endif

/* GenXPow2NTT(ring.AtLevel(level), logN, div)[i] (:772-810): out = NTT(X^(2^i)), or NTT(X^(-2^i)) when div != 0, in Montgomery
 * form, on limbs 0..level of every batch entry of out; 0 <= i < logN */
int he_ring_xpow2_ntt(he_handle ring, int level, int i, int div, he_handle out);
/* The ring maps of Split (:205-225) on one polynomial of degree N, limbs 0..level: outEven = SwitchCiphertextRingDegreeNTT(in),
 * outOdd = SwitchCiphertextRingDegreeNTT(in * XInvPow2NTT[0]), both of degree N/2, as one inverse butterfly per word:
 * outEven[j] = (in[2j] + in[2j+1]) / 2, outOdd[j] = (in[2j] - in[2j+1]) RootsBackward[N/2 + j] / 2.  outOdd may be 0. */
int he_ring_split_ntt(he_handle ringLarge, int level, he_handle in, he_handle outEven, he_handle outOdd /* 0: none */);
/* The ring maps of Merge (:410-417): out = replicate(inEven) + replicate(inOdd) * XPow2NTT[0] as one forward butterfly per word:
 * out[2j] = inEven[j] + w inOdd[j], out[2j+1] = inEven[j] - w inOdd[j], w = RootsForward[N/2 + j].  inOdd may be 0: the replication. */
int he_ring_merge_ntt(he_handle ringLarge, int level, he_handle inEven, he_handle inOdd /* 0: none */, he_handle out);
/* RingPackingEvaluator.Split (:173-228): ctN = (in0, in1) of the evaluator's degree N, the key from the secret of degree N to the
 * one of degree N/2 mapped up; even / odd of degree N/2.  One key switch into scratch (in0 as the ModDown epilogue's addend) and
 * ONE launch of the split over both components.  The inputs are left unchanged.  odd0 and odd1 are both given or both 0. */
int he_ringpack_split(he_handle eval, int level, he_handle in0, he_handle in1, he_handle evk /* N -> N/2 */,
                      he_handle even0, he_handle even1, he_handle odd0, he_handle odd1 /* both 0: none */);
/* RingPackingEvaluator.Merge (:376-426): even / odd of degree N/2, out of the evaluator's degree N.  ONE launch of the merge puts
 * both components into scratch at N, then the key switch runs with the merged component 0 as the addend. */
int he_ringpack_merge(he_handle eval, int level, he_handle even0, he_handle even1, he_handle odd0, he_handle odd1 /* both 0 */,
                      he_handle evk /* N/2 -> N */, he_handle out0, he_handle out1);
/* Expand's inner step at n = 2^k (:528-559) over a batch of m ciphertexts (in, tmp: batch m; tmp = the automorphism of in):
 * out[e] = in[e] + tmp[e] and out[e + m] = (in[e] - tmp[e]) * XInvPow2NTT[k], out of batch 2 m.  sum_only != 0: out (batch m)
 * gets the sums alone, and out_k may be in_k. */
int he_ringpack_expand_step(he_handle ring, int level, int k, int sum_only, he_handle in0, he_handle in1,
                            he_handle tmp0, he_handle tmp1, he_handle out0, he_handle out1);
/* Pack's inner step (:697-765) before the automorphism, over `count` pairs (a, b) of single ciphertexts (batch 1, the ring's
 * degree), x = XPow2NTT[k]; a pair's a (a0[z], a1[z]) or b may be absent (both handles 0), not both.  t0 / t1 of batch count:
 *   a and b: T[z] = a - b x, a <- a + b x;   a only: T[z] = a;   b only: b <- b x, T[z] = b x. */
int he_ringpack_pack_pre (he_handle ring, int level, int k, int count, const he_handle *a0, const he_handle *a1,
                          const he_handle *b0, const he_handle *b1 /* 0 entries = absent */, he_handle t0, he_handle t1);
/* ... and after it (T holds the automorphism's result):  a present: a <- a + T[z];  b only: b <- b - T[z]. */
int he_ringpack_pack_post(he_handle ring, int level, int count, const he_handle *a0, const he_handle *a1,
                          const he_handle *b0, const he_handle *b1, he_handle t0, he_handle t1);

#ifdef __cplusplus
}
#endif
#endif /* HERING_RINGPACK_H */
