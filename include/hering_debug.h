/*
 * hering_debug.h -- diagnostics of libhering.so that are NOT part of the drop-in boundary
 * (include/hering.h): per-kernel timing used by bench.py's roofline leg and an instruction-rate probe.
 * Nothing in the reference corresponds to these; a Go binding does not need them.
 */
#ifndef HERING_DEBUG_H
#define HERING_DEBUG_H

#include "hering.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-kernel HIP-event timing on the context's stream: begin, run work, end -> per kernel id
 * launch counts and summed durations (adds two events per launch).  The state is per context and
 * guarded: other contexts may keep launching from other threads meanwhile and are not recorded. */
int he_prof_begin(he_handle ctx);
int he_prof_end(he_handle ctx, int max_kernels, int *counts, float *total_ms, int *n_kernels);
/* the same, with the summed ALGORITHMIC bytes of the recorded launches per kernel id (every polynomial stream a launch must
 * read or write, once; key rows shared by a batch once; twiddles / constants excluded) -- the numerator of the per-kernel
 * roofline figures; computed by the launchers themselves (csrc/kernels.hip, ProfScope) */
int he_prof_end_bytes(he_handle ctx, int max_kernels, int *counts, float *total_ms, double *total_bytes, int *n_kernels);
const char *he_prof_kernel_name(int id);
/* algorithmic bytes of the primitives called on the context since the last reset, by the per-primitive formulas of
 * SURVEY.md section 8(d) (NTT 2L, binary 3L, GadgetProduct 3L + 2 beta (L + alpha), ... limbs of N * 8 bytes, times the batch):
 * out[0] charges an evaluation key to every batch entry (the section's convention), out[1] reads it once per call */
int he_alg_bytes(he_handle ctx, int reset, double out[2]);
/* modular-multiply work of the primitives called on the context since the last reset, in closed form per primitive (SURVEY.md
 * section 8(d): NTT (N/2) logN + N per limb, basis extension L_src x L_dst x N, key inner product 2 beta (L + alpha) N, tensor 6 L N,
 * ...) and by the arithmetic class of the limb: out[0] multiply-equivalents on integer-class limbs (64-bit Montgomery products),
 * out[1] on limbs below 2^47 (exact double-precision products), out[2] / out[3] how many of these are NTT butterflies */
int he_alg_valu(he_handle ctx, int reset, double out[4]);
/* PCI bus id ("0000:05:00.0") of a HIP device of this process: bench.py finds the device's clock tables in sysfs through it
 * (/sys/bus/pci/devices/<id>/pp_dpm_sclk) -- the node's other GPUs are listed there too, whatever this process may see */
int he_debug_device_pci_bus_id(int device, char *out, int len);
/* dependent-MRedLazy throughput probe: returns modular multiplies per second */
int he_probe_modmul(he_handle ctx, int iters, double *mults_per_s);
/* the same for the exact double-precision product the limbs below 2^47 are computed with (error-free product + rounded quotient,
 * csrc/kernels.hip modmul_f64): the second ceiling of bench.py's `roofline.valu` */
int he_probe_modmul_f64(he_handle ctx, int iters, double *mults_per_s);
/* The scalar arithmetic primitives of the kernels, one by one (csrc/modarith.h and csrc/kernels.hip: the very __device__ functions
 * the production kernels call), each applied to n tuples by one launch of a probe kernel -- one tuple per thread -- with q, qinv,
 * the Barrett constants, NInv and 1/q taken from the ring's RESIDENT constant record of `limb` (so the table builders are under
 * test too).  a, b, c, out0, out1: host arrays of n words; b, c and out1 may be null where the op does not use them (below).
 * Doubles travel as their bit patterns.  HE_EINVAL: unknown op, bad limb, n = 0, n > 2^20, a missing array.
 *   a, b -> out0:        MRED_LAZY, MRED, MRED_LAZY_W32, MRED_LAZY_ASM (x, y); MRED128_LAZY (hi, lo); BRED_LAZY, BRED (x, y);
 *                        MODMUL_F64 (a, w as doubles -> double)
 *   a -> out0:           BRED_ADD[_LAZY], MFORM[_LAZY], IMFORM[_LAZY], HALVE (words); REDUCE_F64, CANON_F64D (double -> double);
 *                        CANON_F64, F64_TO_U52 (double -> word); U52_TO_F64 (word -> double)
 *   a, b, c -> out0, out1: the butterflies on (a, b) with the twiddle c (BFLY_INV_SCALED[_ASM]: c = the twiddle already
 *                        multiplied by N^-1, NInv from the record); the _ASM forms take their product through the hand-written
 *                        sequence of the row kernels
 *   a, b, c -> out0:     AUTO_DEST (e, g^-1 mod 2N, logN) */
enum he_arith_op {
    HE_ARITH_MRED_LAZY = 0, HE_ARITH_MRED, HE_ARITH_MRED_LAZY_W32, HE_ARITH_MRED_LAZY_ASM, HE_ARITH_MRED128_LAZY,
    HE_ARITH_BRED_ADD_LAZY, HE_ARITH_BRED_ADD, HE_ARITH_BRED_LAZY, HE_ARITH_BRED, HE_ARITH_MFORM_LAZY, HE_ARITH_MFORM,
    HE_ARITH_IMFORM_LAZY, HE_ARITH_IMFORM, HE_ARITH_BFLY_FWD, HE_ARITH_BFLY_FWD_ASM, HE_ARITH_BFLY_FWD_NC, HE_ARITH_BFLY_FWD_NC_ASM,
    HE_ARITH_BFLY_INV, HE_ARITH_BFLY_INV_ASM, HE_ARITH_BFLY_INV_SCALED, HE_ARITH_BFLY_INV_SCALED_ASM, HE_ARITH_MODMUL_F64,
    HE_ARITH_REDUCE_F64, HE_ARITH_CANON_F64D, HE_ARITH_CANON_F64, HE_ARITH_U52_TO_F64, HE_ARITH_F64_TO_U52, HE_ARITH_HALVE,
    HE_ARITH_AUTO_DEST, HE_ARITH_COUNT
};
int he_debug_arith(he_handle ring, int limb, int op, size_t n, const uint64_t *a, const uint64_t *b, const uint64_t *c,
                   uint64_t *out0, uint64_t *out1);
/* submission queue of an evaluator (he_evaluator_set_coalescing) since its creation: out[0] = single-ciphertext calls served,
 * out[1] = batched launches made for them, out[2] = largest batch, out[3] = calls that ran one by one because their pipeline
 * has launches without entry tables */
int he_evaluator_coalescing_stats(he_handle eval, uint64_t out[4]);
int he_ctx_coalescing_stats(he_handle ctx, uint64_t out[4]);  /* the same counters through the context handle */
/* diagnosis of the queue's gathering rule since the context was created: out[0..2] = batches launched because every recently
 * active caller was waiting / because the oldest request had waited 8 windows / because max_batch requests were pending; out[3],
 * out[4] = microseconds the leaders spent gathering and launching; out[5] / out[6] = sums of callers present / expected at launch;
 * out[7] = allocations the context's buffer cache could not serve (hipMalloc calls); deferred submission (he_ctx_set_deferred):
 * out[8] = microseconds the dispatcher paused because it was four batches ahead of the device, out[9] / out[10] = microseconds it
 * waited for callers while the device had at least two batches queued (free) / while the device was running dry, out[11] = batches;
 * out[12] (HERING_QUEUE_TIMING=1 only) = device microseconds spent inside the dispatcher's batches; out[13] / out[14] = entry
 * tables filled by a launch / reused from one of the context's table slots (same offsets as a recent batch); out[15] reserved */
int he_debug_queue_counters(he_handle ctx, uint64_t out[16]);
/* per operation of the queue (the CoOp numbering of csrc/api.cpp): out[2 i] = batches launched, out[2 i + 1] = requests served */
int he_debug_queue_op_stats(he_handle ctx, uint64_t out[64]);
/* files a request whose launch fails (HE_EDEVICE) after the call was accepted: in the default mode of the queue the call itself returns
 * the failure; under he_ctx_set_deferred the call returns HE_OK and the next he_ctx_sync reports it (tests) */
int he_debug_queue_inject_failure(he_handle ctx);
/* Concurrent single-ciphertext callers, the shape of the reference's parallel benchmarks (b.RunParallel,
 * schemes/ckks/ckks_benchmarks_test.go:116-207): n_threads OS threads (pthreads inside the library: no interpreter in the timed
 * region); thread i makes `iters` calls on its own batch-1 handles -- op 0: he_ckks_mul_relin(eval[i], level, a0[i], a1[i], b0[i],
 * b1[i], rlk[i], o0[i], o1[i], 0); op 1: he_bgv_mul_relin (t = plaintext modulus); op 2: he_automorphism_ct(eval[i], level, a0[i],
 * a1[i], t = Galois element, rlk[i] = Galois key, o0[i], o1[i]); op 3: he_relinearize(eval[i], level, a0[i], a1[i], b0[i], rlk[i],
 * o0[i], o1[i]); op 4: he_gadget_product(eval[i], level, a0[i], rlk[i], o0[i], o1[i]) (unused handle arrays may repeat another).
 * sync_each != 0: every call is followed by he_ctx_sync(ctx[i]) (a caller that needs each result before its next call),
 * otherwise one sync after the last call.  All threads start together; *wall_s = first start to last finish.  Returns the
 * first non-zero status of any call. */
int he_debug_concurrent_mul_relin(int n_threads, int iters, int sync_each, int op, int level, uint64_t t, const he_handle *ctx,
                                  const he_handle *eval, const he_handle *a0, const he_handle *a1, const he_handle *b0,
                                  const he_handle *b1, const he_handle *rlk, const he_handle *o0, const he_handle *o1,
                                  double *wall_s);

/* A whole circuit under the reference's concurrency shape (BenchmarkConcurrentBootstrap: b.RunParallel over bootstrappers,
 * circuits/ckks/bootstrapping/evaluator_benchmarks_test.go:14-42): n_threads OS threads (pthreads inside the library) each replay
 * `rounds` times a RECORDED sequence of calls of the public entry points of hering.h (lattigo_amd/_lib.py trace_begin / trace_end
 * records one run of a driver; encoding: csrc/replay.cpp).  Handles the recorded run created are replaced by the replaying
 * thread's own; the n_subst handles subst_from[] (the run's inputs) are replaced per thread by subst_to[thread * n_subst + i];
 * every other handle (rings, evaluator, keys, plaintexts) is shared.  watch[]: recorded handles whose per-thread counterparts of
 * the LAST round are returned in watch_out[thread * n_watch + i] and left alive (the caller downloads and frees them).  *wall_s:
 * common start to the last thread's final he_ctx_sync.  Returns the first non-zero status; err (optional) receives its message.
 * The recorder refuses a window that creates a ring, an evaluator or a key (they are shared, not replayed); it leaves out the
 * he_ring_destroy of a ring made before the window, which the host's garbage collector may issue at any time for a ring nothing
 * refers to any more: no call of the window can name that ring. */
int he_debug_replay(he_handle ctx, const uint64_t *program, size_t n_words, int n_threads, int rounds, const uint64_t *subst_from,
                    int n_subst, const uint64_t *subst_to, const uint64_t *watch, int n_watch, uint64_t *watch_out, double *wall_s,
                    char *err, size_t err_len);

/* where the replaying threads spent their time, per function number of the program encoding (csrc/replay.cpp): out[3 f] =
 * microseconds inside the calls of function f summed over the threads, out[3 f + 1] = calls, out[3 f + 2] = longest call */
int he_debug_replay_profile(uint64_t *out, int n_fn, int reset);

/* The schedule he_blind_rotate_core (hering_blindrot.h) follows, computed on the host (csrc/blindrot_plan.h; no device needed).
 * One row a[n_lwe] of words mod 2N, N = 2^logN: the operations BlindRotateCore applies to that row's accumulator, in order, as
 * pairs ops[2 i] = kind (0: Automorphism, 1: ExternalProduct), ops[2 i + 1] = the Galois element / the index of the blind
 * rotation key.  *n_ops receives the length of the list; at most cap pairs are written.  HE_EINVAL for a non-zero even a[i]. */
int he_debug_blindrot_schedule(int logN, const uint64_t *a, int n_lwe, uint64_t *ops, size_t cap, size_t *n_ops);
/* the merged rounds of a batch of rows a[batch][n_lwe]: rounds[(2 r) batch + b] = the Galois element entry b's automorphism of
 * round r takes (0: none), rounds[(2 r + 1) batch + b] = the key of its external product (-1: none).  *n_rounds receives the
 * number of rounds; at most cap rounds are written. */
int he_debug_blindrot_rounds(int logN, const uint64_t *a, int batch, int n_lwe, int64_t *rounds, size_t cap, size_t *n_rounds);

/* The plan he_lintrans_evaluate_many (hering_lintrans.h) follows for one transformation, computed on the host
 * (csrc/lintrans_plan.h; no device needed): n REDUCED, distinct diagonal indices over `slots`, baby-step count N1 (0: the naive
 * form), G giant steps per launch of the grouped kernel (1 .. 4), NthRoot of the ring.  Words: n_groups, n_galois; naive form
 * (n_groups = 0): the position of the zero diagonal or -1; per group: n_members, n_babies, the members (giant steps, ascending),
 * the union of their baby steps (ascending), term[n_babies][n_members] = the position of diagonal j + i in diag[] or -1; then the
 * Galois elements the call asks the key set for (BSGS: the non-zero baby steps, then the non-zero giant steps; naive: the non-zero
 * rotations).  *n_words receives the length; at most cap words are written. */
int he_debug_lintrans_plan(uint64_t nth_root, int slots, int N1, int G, int n, const int *diag, int64_t *out, size_t cap, size_t *n_words);

/* The structure of a polynomial evaluation (hering_polyeval.h), computed on the host (csrc/polyeval_plan.h; no device needed),
 * for a polynomial of `degree` in `basis` with the reference's IsEven / IsOdd / Lazy on a basis that holds the n_powers powers
 * powers[3 i + {0, 1, 2}] = (n, level, ciphertext degree); copy_input: Evaluate (X^1 is copied first) and not
 * EvaluateFromPowerBasis.  Words: log_split, depth, n_leaves, n_steps, the level of the result; per baby step (degree, level,
 * the ciphertext degree it is allocated with, the ciphertext degree of its result, bit k = it has term k); per step, in the
 * order of the reference's primitive calls, (op, destination, level and ciphertext degree of the destination afterwards, the
 * two sources): a power is named by n >= 1 and baby step i by -1 - i; op: 0 CopyNew, 1 Relinearize, 2 Rescale, 3 MulNew,
 * 4 MulRelinNew, 5 Add(x, x), 6 Add(x, -1), 7 Sub, 8 NewCiphertext, 9 Add(res, c_0), 10 MulThenAdd(X[a], c_a, res), 11 Mul,
 * 12 Add.  An evaluation the reference refuses (the level below the depth, no X^1) is HE_EINVAL with its message. */
int he_debug_polyeval_plan(int degree, int basis, int even, int odd, int lazy, int copy_input, int n_powers, const int *powers,
                           int64_t *out, size_t cap, size_t *n_words);

#ifdef __cplusplus
}
#endif
#endif /* HERING_DEBUG_H */
