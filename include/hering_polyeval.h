/*
 * hering_polyeval.h -- polynomial evaluation on a ciphertext: the integer logic of the reference's polynomial.Evaluator
 * (circuits/common/polynomial: OptimalSplit, SplitDegree, the Paterson-Stockmeyer decomposition) on the host, and its baby steps
 * (EvaluatePolynomialVectorFromPowerBasis, polynomial_evaluator.go:254-359) as one fused launch per group of them (libhering.so).
 *
 * The same conventions as hering.h (which this header includes): 0 on success, <0 on error (HE_E*), he_last_error() for the
 * message; outputs are caller-allocated and come last; he_polyeval_leaves files its work on the context's queue (deferred
 * submission included) and records under he_graph_begin / he_graph_end like every other operator entry point.  Its queued
 * requests are served one by one (the kernel takes no entry tables).
 *
 * Operand identity (checked before anything is filed; a rejected call changes no operand): an output that is a power, and two
 * outputs that are one polynomial, are HE_EINVAL.
 *
 * Deliberate differences from the reference:
 *  - Single polynomial only: a PolynomialVector with a slot Mapping is out of scope (a term is a scalar per limb and half; a
 *    plaintext-polynomial operand would take the place of that pair in the table).
 *  - The structure of an evaluation (csrc/polyeval_plan.h) is integer logic and lives in the library; scales and coefficient
 *    values do not: the caller plans them (exact rationals or residues mod t, as everywhere in this project) and supplies
 *    numbers only, which the library checks against its own decomposition.
 *  - Evaluate / EvaluateFromPowerBasis are ONE native call each, but not one request: the call runs the plan step by step, every
 *    step but the baby steps through the operator entry of hering.h that a caller would use (he_ckks_mul_relin / he_bgv_mul_relin,
 *    he_relinearize, he_div_round_by_last_modulus[_many]_ntt, he_add / he_sub, he_double_rns_scalarop), each filing its own request
 *    in the calling thread's order and recording under he_graph_begin / he_graph_end.  Everything that can be refused -- the level
 *    below the depth, a missing relinearization key where the plan relinearizes, an output that is the input or a power, two
 *    outputs that are one polynomial, a basis other than the one the polynomial was planned for, a wrong list of Chebyshev words
 *    -- is refused before the first step is filed: a rejected call changes no operand and no power.
 *  - A Chebyshev Sub meets a power at scale ~s and an unrescaled product at ~s^2; the reference multiplies the smaller operand by
 *    the truncated integer ratio first (evaluateInPlace).  The caller plans that ratio's words like every other scalar
 *    (aux_kind 1 / 2 below).
 */
#ifndef HERING_POLYEVAL_H
#define HERING_POLYEVAL_H

#include "hering.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HE_POLYEVAL_MONOMIAL 0
#define HE_POLYEVAL_CHEBYSHEV 1
#define HE_POLYEVAL_MAX_TERMS 31 /* non-constant terms of one baby step (2^logSplit - 1 with logSplit <= 5) */

/* ---- on the host (no device needed) ------------------------------------------------------------------------------------- */
/* bignum.OptimalSplit (utils/bignum/polynomial.go:14-24): the baby-step width for a polynomial of log_degree bits */
int he_polyeval_optimal_split(int log_degree, int *log_split);
/* SplitDegree (circuits/common/polynomial/power_basis.go:31-49): X^n = X^a * X^b; n <= 0 is the reference's error */
int he_polyeval_split_degree(int n, int *a, int *b);
/* the depth check of Evaluate (polynomial_evaluator.go:62-65): *depth (optional) = ceil(log2 degree); a level below it is
 * HE_EINVAL with the reference's message "%d levels < %d log(d) -> cannot evaluate poly" */
int he_polyeval_depth(int degree, int level, int *depth);

/* the check he_polyeval_poly_create makes of the caller's baby steps (see there), without a ring: HE_EINVAL with a message where
 * their number, a degree or a level differs from the library's decomposition */
int he_polyeval_check_leaves(int degree, int basis, int even, int odd, int lazy, int n_powers, const int *powers, int n_leaves,
                             const int *leaf_degree, const int *leaf_level);

/* ---- Polynomial --------------------------------------------------------------------------------------------------------- */
/* A polynomial of `degree` in `basis` (HE_POLYEVAL_*), with the reference's IsEven / IsOdd (both or neither: no parity filter)
 * and Lazy, planned for a power basis that holds `n_powers` powers: powers[3 i + {0, 1, 2}] = (n, level, ciphertext degree) of
 * each, X^1 among them (a basis without X^1 is the reference's error).  The library derives the decomposition
 * (PatersonStockmeyerPolynomial / recursePS, polynomial.go:62-141) and holds the caller's baby steps against it: n_leaves,
 * leaf_degree[i] and leaf_level[i], in the reference's order (quotients before remainders); a disagreement is HE_EINVAL with a
 * message.  s0 / s1: the scalar words, uploaded here once -- per baby step in order, per coefficient k = 0 .. leaf_degree[i] (those
 * the parity excludes included and ignored), L = 1 + level(X^1) residues: s0 for the coefficients [0, N/2) of a limb, s1 for
 * [N/2, N), the layout of he_double_rns_scalarop (BGV passes the same words twice).  Every word read (limbs up to the baby step's
 * level) must be below its modulus. */
int he_polyeval_poly_create(he_handle ring, int degree, int basis, int even, int odd, int lazy, int n_powers, const int *powers,
                            int n_leaves, const int *leaf_degree, const int *leaf_level, const uint64_t *s0, const uint64_t *s1,
                            he_handle *poly);
int he_polyeval_poly_destroy(he_handle poly);
/* baby steps per launch of the leaf-group kernel: 0 = the library's default (environment HERING_POLYEVAL_GROUP, else built in),
 * 1, 2 or 4.  The words of a result do not depend on it. */
int he_polyeval_poly_set_group(he_handle poly, int G);

/* ---- the baby steps ----------------------------------------------------------------------------------------------------- */
/* EvaluatePolynomialVectorFromPowerBasis (polynomial_evaluator.go:254-359, mapping == nil) for the baby steps
 * [first, first + count) of the polynomial:  out[g] = c_{g,0} + sum_k c_{g,k} X^k  on the limbs 0 .. level_g, the canonical words
 * the reference's Add(res, c_0), MulThenAdd(X[k], c_k, res) for k = deg ... 1 leave.  x[3 (k - 1) + c]: component c of X^k for
 * k = 1 .. n_powers (0: absent; a power of degree 1 has components 0 and 1, a lazy one of degree 2 also 2), NTT domain, every power
 * a baby step uses reaching that baby step's level; out[3 g + c]: component c of the result of baby step first + g, exactly the
 * components it has -- the reference's scalar MulThenAdd resizes its accumulator to the degree of each operand in turn
 * (schemes/ckks/evaluator.go:936, schemes/bgv/evaluator.go:1118), so a result has the degree of the lowest power used and the
 * third component of a higher power is dropped unless every lower one has it; a baby step without terms has degree 1, or 0 when
 * it is the degree-0 remainder of an even polynomial.  All polynomials have the same batch. */
int he_polyeval_leaves(he_handle poly, int first, int count, int n_powers, const he_handle *x, const he_handle *out);

/* ---- PowerBasis --------------------------------------------------------------------------------------------------------- */
/* NewPowerBasis (power_basis.go:17-29) from the degree-1 NTT-domain ciphertext (in0, in1) at `level`: X^1 is a COPY of it.
 * `eval`: the rlwe evaluator the powers are multiplied with.  basis: HE_POLYEVAL_*. */
int he_polyeval_basis_create(he_handle eval, int basis, int level, he_handle in0, he_handle in1, he_handle *pb);
int he_polyeval_basis_destroy(he_handle pb);
/* the powers the basis holds: powers[3 i + {0, 1, 2}] = (n, level, ciphertext degree), ascending n; *n receives their number, at
 * most cap triples are written */
int he_polyeval_basis_powers(he_handle pb, int *powers, size_t cap, size_t *n);
/* the polynomials of X^n: comps[c] = component c or 0.  They belong to the basis (do not free them) and are replaced when a
 * later call relinearizes or rescales the power. */
int he_polyeval_basis_power(he_handle pb, int n, he_handle *comps);
/* The Chebyshev numbers of a run of steps, in the plan's order (he_polyeval_plan): one entry per Add(x, -1) and per Sub.
 * aux_kind[i]: 0 = Add(x, -1) with the words of -1 at that power's scale; 1 / 2 = Sub whose second / first operand is first
 * multiplied by the integer ratio, with the ratio's words; 3 = Sub of operands of one scale (no words read).  aux_s0 / aux_s1:
 * aux_words residues per entry, the layout of he_double_rns_scalarop.  A list that does not match the plan is HE_EINVAL. */
/* PowerBasis.GenPower (power_basis.go:76-160): X^n and what it needs, rescaled.  scheme: 0 CKKS, 1 BGV with plaintext modulus t.
 * rlk: the relinearization key (0: none -- HE_EINVAL where a step relinearizes). */
int he_polyeval_gen_power(he_handle pb, int scheme, uint64_t t, he_handle rlk, int n, int lazy, int n_aux, const int *aux_kind,
                          const uint64_t *aux_s0, const uint64_t *aux_s1, int aux_words);

/* the steps he_polyeval_gen_power runs on a basis that holds `powers`, six words per step as in he_polyeval_plan */
int he_polyeval_gen_power_plan(int basis, int n, int lazy, int n_powers, const int *powers, int64_t *out, size_t cap, size_t *n_words);

/* ---- the evaluation ----------------------------------------------------------------------------------------------------- */
/* Evaluator.EvaluateFromPowerBasis (polynomial_evaluator.go:47-99) of a polynomial planned for exactly the powers the basis holds
 * (he_polyeval_poly_create): the missing powers are generated into the basis, then the baby steps (one he_polyeval_leaves call),
 * the giant steps (EvaluatePatersonStockmeyerPolynomialVector :101-161, EvaluateMonomial :212-251) and the final Relinearize /
 * Rescale, whose result goes to (out0, out1) at the level he_polyeval_plan reports.  LevelsConsumedPerRescaling = 1. */
int he_polyeval_evaluate_from_power_basis(he_handle pb, he_handle poly, int scheme, uint64_t t, he_handle rlk, int n_aux,
                                          const int *aux_kind, const uint64_t *aux_s0, const uint64_t *aux_s1, int aux_words,
                                          he_handle out0, he_handle out1);
/* Evaluator.Evaluate (:33-45) on the ciphertext (in0, in1) at `level`, which is left untouched (X^1 is its copy); the polynomial
 * must have been planned for the basis {X^1 at (level, degree 1)}.  A level below the depth is the reference's error. */
int he_polyeval_evaluate(he_handle eval, he_handle poly, int scheme, uint64_t t, he_handle rlk, int level, he_handle in0, he_handle in1,
                         int n_aux, const int *aux_kind, const uint64_t *aux_s0, const uint64_t *aux_s1, int aux_words, he_handle out0,
                         he_handle out1);
/* The structure of an evaluation, which the callers' planning of scales and words follows: the words of he_debug_polyeval_plan
 * (hering_debug.h, where the format is described). */
int he_polyeval_plan(int degree, int basis, int even, int odd, int lazy, int copy_input, int n_powers, const int *powers, int64_t *out,
                     size_t cap, size_t *n_words);

#ifdef __cplusplus
}
#endif
#endif /* HERING_POLYEVAL_H */
