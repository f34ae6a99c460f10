/*
 * hering_lintrans.h -- plaintext-matrix x ciphertext products by diagonals: the reference's lintrans.Evaluator
 * (circuits/common/lintrans/lintrans_evaluator.go: EvaluateMany :27-79, MultiplyByDiagMatrix :142-274,
 * MultiplyByDiagMatrixBSGS :280-469) and the index of a LinearTransformation (lintrans.go:297-377) (libhering.so).
 *
 * The same conventions as hering.h (which this header includes): 0 on success, <0 on error (HE_E*), he_last_error() for the
 * message; outputs are caller-allocated and come last; the product entries file their work on the context's queue (coalescing,
 * deferred submission) and record under he_graph_begin / he_graph_end like every other operator entry point.  Queued requests of
 * these entries are served one by one (their launches run over contiguous scratch and take no entry tables).
 *
 * Operand identity (checked before anything is filed; a rejected call changes no operand).  With n_lt == 1 the outputs may be
 * the inputs: P * ct, the copy the naive form keeps for its zero diagonal, the decomposition and every pre-rotation are taken
 * before the first output word is written.  With n_lt > 1 no output may be an input.  Two outputs that are the same polynomial,
 * and an output that is a diagonal, are always HE_EINVAL.
 */
#ifndef HERING_LINTRANS_H
#define HERING_LINTRANS_H

#include "hering.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the index, on the host (no device needed) -------------------------------------------------------------------------- */
/* BSGSIndex (lintrans.go:344) of n rotations over `slots` (a power of two) with baby-step count N1 (a power of two): the sorted
 * giant steps rotN1[*n1] and baby steps rotN2[*n2]; each array must have room for min(n, slots) words (null: only the counts).
 * index (optional, 2 n words): per input rotation k, index[2 k] = its giant step and index[2 k + 1] = its baby step. */
int he_lintrans_bsgs_index(const int *diag, int n, int slots, int N1, int *rotN1, int *n1, int *rotN2, int *n2, int *index);
/* FindBestBSGSRatio (lintrans.go:321) with the reference's float64 comparisons restated exactly, `ratio == maxRatio` and the
 * Inf / NaN of a zero count included. */
int he_lintrans_find_best_bsgs_ratio(const int *diag, int n, int maxN, int logMaxRatio, int *N1);
/* GaloisElements (lintrans.go:297) on the evaluator's ring (NthRoot = 2N, 4N on a conjugate-invariant ring); logBSGSRatio < 0:
 * the naive form.  At most cap elements are written; *n_out receives their number. */
int he_lintrans_galois_elements(he_handle eval, const int *diag, int n, int slots, int logBSGSRatio, uint64_t *out, size_t cap,
                                size_t *n_out);

/* ---- LinearTransformation ----------------------------------------------------------------------------------------------- */
/* n encoded diagonals (NTT + Montgomery, as lintrans.Encode leaves them): diag[k] is the index of (ptQ[k], ptP[k]), polynomials
 * of one entry with at least levelQ + 1 and levelP + 1 limbs.  slots = 2^log_slots (LogDimensions.Cols).  N1 = 0: the naive form
 * (MultiplyByDiagMatrix); N1 a power of two: the baby-step giant-step form.  Indices are reduced as the reference reduces them
 * (& (slots - 1), a negative index + slots); two that reduce to the same rotation are HE_EINVAL.  The handle keeps the diagonal
 * polynomials alive and copies no words: they are read when the transformation is evaluated.  The plan (csrc/lintrans_plan.h)
 * is built and its term table uploaded here. */
int he_lintrans_create(he_handle eval, int levelQ, int levelP, int log_slots, int N1, int n, const int *diag, const he_handle *ptQ,
                       const he_handle *ptP, he_handle *lt);
int he_lintrans_destroy(he_handle lt);
/* giant steps per launch of the grouped kernel: 0 = the library's default (environment HERING_LINTRANS_GROUP, else built in),
 * 1, 2 or 4; later evaluations follow the plan of that grouping (the handle holds one per G, so that one process can run every
 * grouping).  A call lowers G where the group block would outgrow the rest of its scratch.  The words of a
 * result do not depend on it. */
int he_lintrans_set_group(he_handle lt, int G);

/* ---- evaluation --------------------------------------------------------------------------------------------------------- */
/* Evaluator.EvaluateMany on the degree-1 NTT-domain ciphertext (in0, in1) at ct_level: (out0[k], out1[k]) = lts[k] x ct.
 * galois_set: he_galois_keyset_create (hering_blindrot.h) holding every element the transformations need (0: no set, for
 * transformations of the zero diagonal alone, which need no key) -- a missing one, a key whose LevelP differs from the
 * transformations', a key in base-2 form where the hoisted method needs plain digits, or a transformation whose LevelP differs
 * from the first one's is HE_EINVAL.
 * One DecomposeNTT at levelQ = min(max_k LevelQ_k, ct_level); the pre-rotations (AutomorphismHoistedLazy) at that level, shared
 * by the transformations of the call; transformation k works at min(limbs(out0[k]) - 1, ct_level, LevelQ_k).  Outputs are
 * canonical and equal, word for word, to the reference's. */
int he_lintrans_evaluate_many(he_handle eval, he_handle galois_set, int ct_level, he_handle in0, he_handle in1, int n_lt,
                              const he_handle *lts, const he_handle *out0, const he_handle *out1);
int he_lintrans_evaluate(he_handle eval, he_handle galois_set, int ct_level, he_handle in0, he_handle in1, he_handle lt,
                         he_handle out0, he_handle out1);

#ifdef __cplusplus
}
#endif
#endif /* HERING_LINTRANS_H */
