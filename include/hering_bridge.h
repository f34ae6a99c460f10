/*
 * hering_bridge.h -- the CKKS DomainSwitcher (schemes/ckks/bridge.go) and the two ring maps under it
 * (ring/conjugate_invariant.go:3-44) (libhering.so).
 *
 * The same conventions as hering.h (which this header includes): 0 on success, <0 on error (HE_E*), he_last_error() for the
 * message; outputs are caller-allocated and come last; every entry files its work on the context's queue (coalescing, deferred
 * submission) and records under he_graph_begin / he_graph_end like every other operator entry point.
 *
 * Degrees.  A standard polynomial of degree N = 2n in Z[X]/(X^N+1) and a conjugate-invariant one of degree n >= 16, the
 * compressed form of Z[X+X^-1]/(X^N+1): exactly a factor of two (HE_EINVAL otherwise).  A poly handle does not carry its moduli:
 * both sides hold residues of the same moduli, limb for limb (a standard ring of degree N and a conjugate-invariant ring of degree
 * N/2 both need q = 1 mod 2N).  Batches must match (HE_EINVAL).
 *
 * Operand identity (checked before anything is filed; a rejected call changes no operand): handles of different degree cannot
 * coincide, so the only pair that can is out0 == out1 of the ciphertext entries, which is HE_EINVAL; in0 == in1 is accepted.
 */
#ifndef HERING_BRIDGE_H
#define HERING_BRIDGE_H

#include "hering.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ring.UnfoldConjugateInvariantToStandard (ring/conjugate_invariant.go:7): polyStandard[j] = polyStandard[N-1-j] =
 * polyConjugateInvariant[j] for j < n, on limbs 0..level */
int he_unfold_conjugate_invariant_to_standard(int level, he_handle polyConjugateInvariant, he_handle polyStandard);
/* ring.FoldStandardToConjugateInvariant (ring/conjugate_invariant.go:28) on limbs 0..level:
 * polyConjugateInvariant[j] = CRed(polyStandard[N-1-j] + polyStandard[j], q) for j < n, the 64-bit sum wrapping as the
 * reference's does on lazy words.  `ring` supplies the moduli: a ring of either type of degree n or 2n (the reference's receiver
 * is the conjugate-invariant ring of degree n; only its moduli and N() are used).  The entry takes no index table: it is defined
 * for the table of the Galois element NthRoot - 1 = 2N - 1, AutomorphismNTTIndex(N, 2N, 2N-1)[j] = N-1-j, the only one the
 * reference ever passes (bridge.go:41). */
int he_fold_standard_to_conjugate_invariant(he_handle ring, int level, he_handle polyStandard, he_handle polyConjugateInvariant);
/* ckks.DomainSwitcher.ComplexToReal (bridge.go:57-95), NTT-domain degree-1 ciphertexts: in of the evaluator's degree N, out of
 * degree N/2.  (t0, t1) = GadgetProduct(in1) + (in0, 0) at min(level, the key's level), out_k = Fold(t_k).  The evaluator must be
 * on a standard ring.  The scale of the result is twice the input's (bridge.go:93): the caller's to record. */
int he_complex_to_real(he_handle eval, int level, he_handle in0, he_handle in1, he_handle evk, he_handle out0, he_handle out1);
/* ckks.DomainSwitcher.RealToComplex (bridge.go:104-144): in of degree N/2, out of the evaluator's degree N.
 * u_k = Unfold(in_k), (out0, out1) = GadgetProduct(u1) + (u0, 0). */
int he_real_to_complex(he_handle eval, int level, he_handle in0, he_handle in1, he_handle evk, he_handle out0, he_handle out1);

#ifdef __cplusplus
}
#endif
#endif /* HERING_BRIDGE_H */
