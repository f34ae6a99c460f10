// kernels.h -- host-callable launchers of the gfx950 kernels (implemented in kernels.hip).
// All launchers enqueue on the given stream and return the hipError_t of the launch.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdlib>

#include "modarith.h"

namespace he {

// run-time switch HERING_* (DESIGN.md section 9): set and non-zero
inline bool env_flag(const char *name) {
    const char *v = std::getenv(name);
    return v != nullptr && std::atoi(v) != 0;
}
constexpr int kMaxLimbs = 64;  // limbs addressed by one launch
constexpr int kMaxLogN = 20;   // the reference's MaxLogN (core/rlwe/params.go:21); the fused key-switch pipelines cover logN <= 17

// Which limbs a launch touches: entry y of the grid's y-dimension reads limb in_limb[y]
// of the input view(s), writes limb out_limb[y] and uses modulus record mod[y].
struct LimbTab {
    int n;
    uint8_t in_limb[kMaxLimbs];
    uint8_t out_limb[kMaxLimbs];
    uint8_t mod[kMaxLimbs];
};

// A device-resident polynomial batch: limb stride N words, batch stride bstride words.
// tab (optional): an entry table -- batch entry z lives at p + tab[z] words (a device array of word offsets, any allocation;
// differences wrap modulo 2^64) instead of p + z * bstride.  That is how concurrent single-ciphertext calls are coalesced into
// one batched launch over the callers' own, unrelated polynomials (he_evaluator_set_coalescing).  Only the launchers that
// say so accept it -- the caller-facing operands of the fused MulRelin / key-switch pipelines: launch_tensor; the input, the
// product prologue and the epilogues of launch_ntt_rows; the own-digit operand of launch_ks_inner / launch_ntt_mac_f64 and the
// latter's epilogue; the output of launch_gather -- every other launcher refuses a view that carries one.
struct View {
    uint64_t *p;
    size_t bstride;
    const size_t *tab = nullptr;
};
// fills a device entry table from host values (kernel arguments: no host buffer has to outlive the call)
hipError_t launch_tab_fill(size_t *dst, const size_t *vals, int n, hipStream_t s);

struct RingDev {
    int logN;
    int N;
    const ModConst *mc;      // [n_mod]
    const uint64_t *tw_fwd;  // [n_mod][N] RootsForward  (Montgomery form, bit-reversed order)
    const uint64_t *tw_inv;  // [n_mod][N] RootsBackward
    // HOST array [n_mod], kernel class per modulus: 2 = below 2^47 (double-precision row kernel),
    // 1 = below 2^58 (correction-free integer butterflies), 0 = generic
    const uint8_t *host_small;
    const double *twd_fwd;      // [n_mod][N] plain twiddles as doubles (entries of class-2 moduli only), or null
    const double *twd_inv;
    // [n_mod][16][2]: {w, floor(w 2^64 / q)} for the plain (non-Montgomery) forward twiddles RootsForward[0..15] -- the column
    // stages fused into the basis extension use Shoup products on the integer path; null when not built
    const uint64_t *tws_fwd = nullptr;
};

// ---- NTT ---------------------------------------------------------------------------
enum NttFlags {
    NTT_REDUCE_INPUT = 1,  // inputs are arbitrary 64-bit words: bring them to [0,2q) first
    NTT_LAZY_OUT = 2,      // forward: leave the output in [0,2q) instead of [0,q)
    NTT_ADD_SCALAR = 4,    // (set by launch_ntt when io_scalar is given)
    NTT_INPUT_F64 = 8,     // launch_ntt_rows, forward: the limbs of the double-precision class hold doubles (launch_modup_fused f64_raw)
};
struct NttEpilogue;
// io_scalar (optional, one word per launch limb): forward -- added to the input words before the transform (lazy, then reduced when
// NTT_REDUCE_INPUT is set); inverse -- out = CRed(INTT(in) + s).  epi (optional, forward only): the epilogue of
// launch_ntt_rows on the last pass.  Together they make DivRoundByLastModulusNTT two transforms (ring/scaling.go:101-122).
hipError_t launch_ntt(const RingDev &r, const LimbTab &tab, View in, View out, int batch, bool inverse, int flags,
                      hipStream_t s, const uint64_t *io_scalar = nullptr, const NttEpilogue *epi = nullptr);
// only the contiguous-row pass (the last min(logN,12) forward stages / the first ones of the inverse);
// the strided column stages are then done by the producer / consumer kernel (launch_modup_fused).
// For logN <= 12 this is the whole transform (inverse: N^-1 included).
// Optional epilogue of the forward row pass = the last op of ModDownQPtoQNTT (ring/basis_extension.go:252-255),
// optionally fused with the Ring.Add every key-switch caller applies next:
//   out = [w +] MRed(NTT(in) + 2q - y, s[limb])      (y, w, out indexed by tab.out_limb)
struct NttEpilogue {
    View y, w;
    bool has_w;
    uint64_t s[kMaxLimbs];
    // the limbs handled by the double-precision kernel hold y as IEEE doubles (integers, |y| < q) -- the accumulators
    // ntt_mac_f64 wrote with q_out_f64
    bool y_small_f64 = false;
    // y is caller-supplied (arbitrary 64-bit words): the double-precision kernel reduces it before converting
    bool y_reduce = false;
    // optional second output set: batch entries >= zsplit use (out2, y2, w2) with index z - zsplit
    // (both components of a ciphertext in one launch)
    int zsplit = 0;
    View out2, y2, w2;
    bool has_w2 = false;
    // tensor mode (fused MulRelin; launch_ntt_rows with zsplit = B): the addend of a component is formed from the four
    // inputs of the ciphertext product instead of being read back -- w0 = T(a0, b0), w1 = CRed(T(a0, b1) + T(a1, b0)),
    // T(x, y) = MRed(MRed(x, ts[limb]), y) (schemes/bgv/evaluator.go:634-647) -- and the two components of an entry are given
    // workgroups eight apart in launch order (the same XCD, back to back), so that the second one finds a0 / b0 in that L2
    bool tensor = false;
    View ta0, ta1, tb0, tb1;
    uint64_t ts[kMaxLimbs];
    // launch_ntt only: the epilogue pass writes here instead of `out` (which then only carries the column pass's
    // intermediate), so that dst may alias y
    bool has_dst = false;
    View dst;
    // launch_ntt_rows, not with `tensor`: the result is stored through the NTT-domain automorphism of Galois element g (ring/
    // automorphism.go:50-77: coefficient e of the transform lands where out[j] = in[index_g[j]] reads it); scatter_ginv = g^-1 mod 2N
    // (standard ring), 0 = plain stores.  Outputs must then not alias the addends (a thread reads w at e and writes elsewhere).
    uint32_t scatter_ginv = 0;
};
// Optional prologue of the INVERSE row pass over the limbs of the double-precision class (production row sizes): the input is
// formed in the kernel as the degree-2 term of a ciphertext product, c = T(a, b) = MRed(MRed(a, ts[limb]), b), canonical, and
// also written to `c` (limb-indexed like `in`) -- the tensor pass over those limbs and the read-back of its output disappear.
// The integer-class limbs of the launch read `in` as usual (the caller's tensor pass covers them).  ts by tab position.
struct NttProdIn {
    View a, b, c;
    uint64_t ts[kMaxLimbs];
};
int ntt_row_bits(int logN);  // row stages of the two-pass transform (the rest are column stages)
bool ntt_prod_in_supported(int logN);
bool epilogue_scatter_supported(int logN);  // NttEpilogue::scatter_ginv / NttMacEpilogue::scatter_ginv: the production row sizes
hipError_t launch_ntt_rows(const RingDev &r, const LimbTab &tab, View in, View out, int batch, bool inverse, int flags,
                           hipStream_t s, const NttEpilogue *epi = nullptr, const NttProdIn *prod = nullptr);

// conjugate-invariant fold (ring/ntt.go:764-769 forward, :1146-1151 backward), pairs (j, N-j) per thread:
//   forward : out[j] = in[j] + 2q - MRedLazy(in[N-j], F), out[0] = in[0]          (F = ModConst.pad0)
//   backward: out[j] = CRed(in[j] + q - MRed(in[N-j], F)), out[0] = 2*in[0] mod q  (F = ModConst.pad1, in canonical)
hipError_t launch_ci_fold(const RingDev &r, const LimbTab &tab, View in, View out, int batch, bool inverse, bool reduce_input,
                          hipStream_t s);

// INTTConjugateInvariantLazy of ONE limb with the reference's exact lazy words (see kernels.hip); `in` / `out` address that limb
// (limb stride folded into the pointer), mc_host is the host copy of the modulus record
hipError_t launch_ci_intt_lazy_ref(const RingDev &r, const ModConst &mc_host, int mod, View in, View out, int batch, hipStream_t s);

// ---- coefficient-wise -----------------------------------------------------------------
// op codes: 0..16 = he_binop, 100.. = he_unop, 200.. = scalar forms (scalar per limb in sc[])
enum EwOp {
    EW_ADD = 0, EW_ADD_LAZY, EW_SUB, EW_SUB_LAZY,
    EW_MUL_BARRETT, EW_MUL_BARRETT_LAZY, EW_MUL_BARRETT_THEN_ADD, EW_MUL_BARRETT_THEN_ADD_LAZY,
    EW_MUL_MONT, EW_MUL_MONT_LAZY, EW_MUL_MONT_LAZY_THEN_NEG,
    EW_MUL_MONT_THEN_ADD, EW_MUL_MONT_THEN_ADD_LAZY, EW_MUL_MONT_LAZY_THEN_ADD_LAZY,
    EW_MUL_MONT_THEN_SUB, EW_MUL_MONT_THEN_SUB_LAZY, EW_MUL_MONT_LAZY_THEN_SUB_LAZY,
    EW_NEG = 100, EW_REDUCE, EW_REDUCE_LAZY, EW_MFORM, EW_MFORM_LAZY, EW_IMFORM, EW_COPY,
    EW_ZERO,                       // 0 (no input read: the zero fill of a batch of fresh polynomials through an entry table)
    EW_ADD_SCALAR = 200,           // CRed(x + s)
    EW_SUB_SCALAR,                 // CRed(x + q - s)
    EW_MUL_SCALAR_MONT,            // MRed(x, s)
    EW_MUL_SCALAR_MONT_THEN_ADD,   // CRed(z + MRed(x, s))
    EW_ADD_SCALAR_LAZY,            // x + s
    // rescale / moddown fused forms (two-limb inputs)
    EW_SUB_THEN_MUL_SCALAR_MONT_2Q = 300,  // z = MRed(2q - y + x, s)          vec_ops.go:766
    EW_DIVROUND_COEFF,                     // z = MRed(x + (s0 + 2q - y), s)    scaling.go:138-142 (x = top limb + pHalf)
    EW_SUBMUL2Q_THEN_ADD,                  // z = CRed(z + MRed(2q - y + x, s)): ModDown epilogue fused with Ring.Add
};
struct ScalarTab {
    uint64_t s[kMaxLimbs];   // per launch-limb scalar
    uint64_t s2[kMaxLimbs];  // second scalar where needed
};
// z[out_limb] = op(x[in_limb], y[in_limb or y_limb], z)   (y uses tab.in_limb unless y_tab given)
hipError_t launch_ew(const RingDev &r, const LimbTab &tab, int op, View x, View y, View z, int batch,
                     const ScalarTab *sc, const uint8_t *x_limb_override, hipStream_t s);
// "double scalar" forms (Ring.{Add,Sub,Mul}DoubleRNSScalar, ring/operations.go:166-184,249-268): sc->s for the
// coefficients [0, N/2), sc->s2 for [N/2, N); op is one of the scalar EW ops
hipError_t launch_ew_double(const RingDev &r, const LimbTab &tab, int op, View x, View z, int batch, const ScalarTab *sc,
                            hipStream_t s);
// Ring.Shift (operations.go:279: out[j] = in[(j + k) mod N], k already reduced to [0, N)) and Ring.MultByMonomial
// (:307: p2 = p1 * X^k in Z[X]/(X^N+1), word-exact incl. the q - 0 = q representative), shift in [0, 2N); not in place
hipError_t launch_shift(const RingDev &r, const LimbTab &tab, View in, int k, View out, int batch, hipStream_t s);
hipError_t launch_mult_by_monomial(const RingDev &r, const LimbTab &tab, View in, int shift, View out, int batch, hipStream_t s);
// same with a separate addend view w for the *_THEN_ADD forms (z = f(x, y) + w)
hipError_t launch_ew_w(const RingDev &r, const LimbTab &tab, int op, View x, View y, View w, View z, int batch,
                       const ScalarTab *sc, hipStream_t s);

// ---- automorphism ------------------------------------------------------------------------
hipError_t launch_gather(const RingDev &r, const LimbTab &tab, View in, const uint32_t *index, View out, int batch,
                         bool then_add, hipStream_t s);
// coefficient-domain automorphism X^i -> X^(i*gal) (ring/automorphism.go:153-174)
hipError_t launch_automorphism_coeff(const RingDev &r, const LimbTab &tab, View in, uint64_t gal, View out, int batch,
                                     hipStream_t s, bool conjugate_invariant = false);
// lognth = log2(NthRoot) - 1: logN for the standard ring, logN + 1 for the conjugate-invariant one
hipError_t launch_build_automorphism_index(int logN, int lognth, uint64_t gal, uint32_t *index, hipStream_t s);

// ---- basis extension -----------------------------------------------------------------------
// One constant set of GenModUpConstants (ring/basis_extension.go:101) resident on the device.
struct ModUpDev {
    int nsrc, ndst;
    const uint64_t *a;         // [nsrc]           qoverqiinvqi
    const uint64_t *T;         // [ndst][nsrc]     qoverqimodp
    const uint64_t *vt;        // [ndst][nsrc+1]   vtimesqmodp
};
struct ModUpArgs {
    int nsrc, ndst;
    uint8_t src_limb[32], src_mod[32];
    uint64_t src_half[32];               // added (CRed) before reconstruction; 0 = none
    uint8_t dst_limb[kMaxLimbs], dst_mod[kMaxLimbs], dst_row[kMaxLimbs];
    uint64_t dst_half[kMaxLimbs];        // subtracted (CRed(x + p - half)) after
    uint8_t dst_view[kMaxLimbs];         // 0 -> dstA, 1 -> dstB
};
hipError_t launch_modup(const RingDev &r, const ModUpDev &c, const ModUpArgs &a, View src, View dstA, View dstB,
                        int batch, hipStream_t s);
// single-limb digit: centred copy into every listed limb (ring/basis_extension.go:402-436)
// strict bit 0: the sign test is c > q/2 instead of c >= q/2 (circuits/ckks/bootstrapping/evaluator.go:681 vs :657);
// bit 1: |c| is written unreduced (ringqp.Ring.ExtendBasisSmallNormAndCenter, ring/ringqp/operations.go:325)
hipError_t launch_center_copy(const RingDev &r, const ModUpArgs &a, View src, View dstA, View dstB, int batch,
                              hipStream_t s, int strict = 0);

// Fused basis extension for the key-switch pipelines: [last `a` inverse-NTT stages + N^-1 on the
// sources] -> ModUpExact (or the centred copy of a one-limb digit) -> [first `a` forward-NTT stages on
// every destination limb], a = logN - 12.  Sources are the output of the inverse ROWS pass, destinations
// feed the forward ROWS pass, so the strided "column" passes never touch HBM on their own.
// One descriptor per digit, resident in device memory (built once per (levelQ, levelP) plan).
#ifndef HE_MODUP_MAGIC
#define HE_MODUP_MAGIC 1  // split residues: exact running sum of the products, one reduction per coefficient (0: one modmul_f64 each)
#endif
// a source residue of 2^51 and above is split y = yh 2^kYSplitBits + yl for the double-precision destinations (both halves fit
// 32 bits for moduli below 2^61)
constexpr int kYSplitBits = HE_MODUP_MAGIC ? 29 : 26;
#ifndef HE_MODUP_R60
#define HE_MODUP_R60 1  // 0: the lean integer destinations always assemble their 128-bit sum (dst_fast 1)
#endif
struct ModUpDesc {
    int nsrc, ndst, single, reduce_out;
    const uint64_t *a, *T, *vt;
    // double-precision copies for destination moduli below 2^47: Td[row][i] = {T, T*2^kYSplitBits mod p} (plain integers),
    // vtd[row][v] = vt; a source residue y >= 2^51 is split as y = yh*2^kYSplitBits + yl (src_split[i])
    const double *Td, *vtd;
    // lean integer path (destination moduli below 2^58, see modup_fused_kernel): fc[row] = {vt[row][1] 2^64 mod p,
    // (p - dst_half) 2^64 mod p}; dst_fast[j] marks the destinations that take it
    const uint64_t *fc;
    // dst_fast = 3: the lean path with the sum reduced at radix 2^30; t60[row] = {T[i] 2^60 mod p (nsrc of them), vt[1] 2^60 mod p,
    // (p - dst_half) 2^60 mod p}
    const uint64_t *t60;
    uint8_t dst_fast[kMaxLimbs];
    uint8_t src_split[8];
    uint64_t src_half[8];
    uint8_t src_limb[8], src_mod[8];
    size_t dst_off;  // words added to the destination bases (digit block)
    uint8_t dst_limb[kMaxLimbs], dst_mod[kMaxLimbs], dst_row[kMaxLimbs], dst_view[kMaxLimbs];
    uint64_t dst_half[kMaxLimbs];
};
// all descriptors must share nsrc; returns hipErrorInvalidValue when (nsrc, logN) has no fused kernel
bool modup_fused_supported(int logN, int nsrc);
// dst_classes: bit 0 = some destination modulus is >= 2^47 (integer path), bit 1 = some is below (double path)
// total_limbs: source + destination limbs over the descriptors (the launch's algorithmic traffic, for the profiling leg)
hipError_t launch_modup_fused(const RingDev &r, const ModUpDesc *descs_dev, int ndesc, int nsrc, int dst_classes, View src,
                              View dstA, View dstB, int batch, hipStream_t s, bool f64_raw = false, int total_limbs = 0);
// f64_raw is exact only while the unreduced doubles stay below 2^53 through the remaining forward stages
bool modup_f64_raw_ok(int logN, int nsrc, uint64_t max_small_modulus);

// base-2 gadget decomposition (ring.MaskVec, ring/vec_ops.go:870, as used by
// core/rlwe/evaluator_gadget_product.go:256-258): block b = (RNS digit i, window j) gets
// (src[limb_i] >> shift_b) & mask replicated into every listed destination limb
struct MaskSpreadArgs {
    int nblk, ndst;
    uint64_t mask;
    uint8_t blk_limb[256], blk_shift[256];
    uint8_t dst_limb[kMaxLimbs];
};
hipError_t launch_mask_spread(const RingDev &r, const MaskSpreadArgs &a, View src, uint64_t *dec, size_t dec_bs, size_t dec_ds,
                              int batch, hipStream_t s);

// ---- the fused gadget product of a small ring: one kernel (gadget_fused_kernel), two tails --------
// RGSW external product (core/rgsw/evaluator.go:130-204), the whole product of one batch entry in one workgroup: out_c = [ModDown of] sum over (component k, source
// limb i, window j) of key_k[prefix[i] + j][c] * NTT((INTT(in_k)[i] >> j pw2) & mask), limbs 0..nQ-1, canonical.  Standard rings,
// at most one special prime (nP; its modulus record is p_mod and its limb inside a key block key_p_limb).  out_k may be in_k.
// ktab (select form): a device array [2][nkeys] of key base addresses (rgsw0 | rgsw1) and sel, a device array of one int32 per
// batch entry: the entry's key, or -1 = the entry is copied.
constexpr int kRgswMaxQ = 8;
struct RgswFusedArgs {
    View in0, in1, out0, out1;  // no entry tables
    const uint64_t *key0 = nullptr, *key1 = nullptr;
    const size_t *ktab = nullptr;
    const int32_t *sel = nullptr;
    int nkeys = 0;
    int nQ = 0, nP = 0, p_mod = 0, key_limbs = 0, key_p_limb = 0;
    int pw2 = 0;                // 0: one uncentred window per limb, mask = all ones
    uint64_t mask = 0;
    uint8_t nj[kRgswMaxQ], prefix[kRgswMaxQ];
    uint64_t md_s[kRgswMaxQ];     // q_u - MForm(P^-1 mod q_u)
    uint64_t p_mod_q[kRgswMaxQ];  // p mod q_u
    uint64_t p_half = 0;          // (p - 1) / 2
};
bool rgsw_fused_supported(int logN, int nQ);  // logN 9..11 and the coefficients of 2 nQ limbs beside the exchange buffer in 64 KiB of LDS
hipError_t launch_rgsw_fused(const RingDev &r, const RgswFusedArgs &a, int batch, hipStream_t s);
// rlwe.Evaluator.Automorphism (core/rlwe/evaluator_automorphism.go:13-56) of one batch entry in one workgroup: the same kernel
// decomposing in1 alone, with the tail out = permute(acc + (in0, 0)).  Select form only: entry b takes key sel[b] of the set, or
// is copied (sel[b] == -1).  Same domain and arguments as launch_rgsw_fused with a base-2 gadget key (pw2 != 0); key0 / key1 are
// not read and ktab is a device array [2][nkeys]: the keys' base addresses | the addresses of their automorphism index tables
// (uint32 [N], out[j] = in[index[j]]).  out_k may be in_k.
hipError_t launch_auto_fused(const RingDev &r, const RgswFusedArgs &a, int batch, hipStream_t s);

// ---- key-switch inner product ---------------------------------------------------------------
// acc[k][l] = sum_d evk[d][k][l] * dec[d][l] * 2^-64 mod q_l, canonical
// (core/rlwe/evaluator_gadget_product.go:160-200 after its final Reduce).
struct KsArgs {
    int beta;
    int nlimbs;                       // launch limbs
    uint8_t dec_limb[kMaxLimbs];      // limb inside one digit block of dec
    uint8_t key_limb[kMaxLimbs];      // limb inside one (d,k) block of the key
    uint8_t out_limb[kMaxLimbs];
    uint8_t out_view[kMaxLimbs];      // 0 -> Q outputs, 1 -> P outputs
    uint8_t mod[kMaxLimbs];
    size_t dec_dstride;               // words between digits in dec
    size_t key_kstride;               // words between k=0 and k=1 blocks
    size_t key_dstride;               // words between digits in the key
    // optional: the digit's own limbs are read straight from the NTT-domain input instead of dec
    // (core/rlwe/evaluator_gadget_product.go:498-503 copies them); alpha = 0 disables
    int own_alpha;                    // digit d owns Q limbs [d*alpha, (d+1)*alpha)
    int own_nq;                       // launch limbs < own_nq are Q limbs with limb index == launch index
};
// Optional (AutomorphismHoistedLazy as ONE launch, core/rlwe/evaluator_automorphism.go:104-165): the accumulators are stored
// through the NTT-domain automorphism whose inverse Galois element is ginv (see NttEpilogue::scatter_ginv), and component 0 of
// the Q limbs is first increased by MRed(add0, add_s[launch limb]) -- the ctIn[0] * P term -- read at the source position.
// Round 6 -- the giant step of a baby-step giant-step linear transformation (circuits/common/lintrans/lintrans_evaluator.go:
// 397-441: GadgetProductLazy, ringQP.Add of the inner loop's component-0 sum, AutomorphismNTTWithIndex[ThenAddLazy] of both
// components into the outer accumulators) as the producers' own stores: `plain` -- the addend (add0 on the Q limbs, add0P on
// the P limbs) is added as it is, CRed(acc + add); `accumulate` -- the destination word is increased (no reduction, as
// ...ThenAddLazy) instead of overwritten.  launch_ntt_mac_f64 takes the same description for the double-precision limbs.
struct KsScatter {
    uint32_t ginv = 0;
    View add0{nullptr, 0};
    uint64_t add_s[kMaxLimbs];
    int plain = 0;
    View add0P{nullptr, 0};
    int accumulate = 0;
};
hipError_t launch_ks_inner(const RingDev &r, const KsArgs &a, View dec, View own, const uint64_t *key, View out0Q,
                           View out0P, View out1Q, View out1P, int batch, hipStream_t s, const KsScatter *sc = nullptr);

// Plaintext-diagonal x ciphertext multiply-accumulate (inner loop of lintrans, circuits/common/lintrans/
// lintrans_evaluator.go:346-394): out_k = Reduce(prev_k + sum_i MulCoeffsMontgomeryLazy(pt_i, ct_i[k])), k = 0,1, for the
// limbs [0, nlimbs) of one ring; exact 128-bit accumulation and one Montgomery reduction, i.e. the canonical value of the
// reference's lazy accumulation after its final Reduce.  pt_i is shared by the batch (bstride 0) or per entry; a term may
// be read through an automorphism index (gather), which fuses AutomorphismNTTWithIndex into the product.
constexpr int kMaxDiag = 64;
struct DiagMacArgs {
    int n, nlimbs, accumulate;
    int mod0;                                                    // modulus record of limb 0 in the ring's table
    const uint64_t *pt[kMaxDiag], *c0[kMaxDiag], *c1[kMaxDiag];  // c0/c1 null: the term is skipped on this ring
    const uint32_t *index[kMaxDiag];                             // null: identity
    size_t pt_bs[kMaxDiag], c0_bs[kMaxDiag], c1_bs[kMaxDiag];
    // optional entry tables of the terms' operands (View::tab for a term list): row term_rows * i + {0: pt, 1: c0, 2: c1} of
    // term_tab holds, per batch entry, the word offsets from the term's base pointers; replaces the batch strides
    const size_t *term_tab = nullptr;
    int term_rows = 3;
};
hipError_t launch_diag_mac(const RingDev &r, const DiagMacArgs &a, View out0, View out1, int batch, hipStream_t s);

// The inner sums of a GROUP of giant steps of MultiplyByDiagMatrixBSGS in one pass over the pre-rotated ciphertexts
// (he_lintrans_evaluate_many): per member g of the group and component k,
//   out[g][k] = CRed(MRedLazy128(sum_i pt_{j_g + i} * ct_i[k]))      over the baby steps i of the group's union,
// the canonical words launch_diag_mac writes for that giant step alone.  Each ct_i is loaded once per group (non-temporal) and
// multiplied into the accumulators of every member that has diagonal j_g + i.
// Term table (device, built once per transformation): per baby step of the group a row of `row_words` = 1 + 2 members words,
//   row[0] = source of ct_i: 0 = the P * ct block (`pct`, the i = 0 term: skipped where pct is null, it has no P part), s > 0 =
//            pre-rotation s - 1 of the transformation's own list, mapped through slot_map (null: identity) to a slot of `ct`;
//   row[1 + 2 g], row[2 + 2 g] = address of the Q and of the P words of member g's diagonal (0: the member has no such term).
// ct: [slot][2][batch] polynomials (ct_comp = words between the components, ct_slot between slots, ct_bs between entries); pct
// and out likewise ([2][batch] and [member][2][batch]).  One launch per ring part over a grid of (N / 256, limbs, ceil(batch / BB)).
constexpr int kDiagGroupMax = 4;
struct DiagMacGroupArgs {
    const uint64_t *tab;
    int n_babies, members, row_words, part;  // part: 0 = Q words of the diagonals, 1 = P words
    const uint64_t *slot_map;
    const uint64_t *ct, *pct;
    size_t ct_slot, ct_comp, ct_bs, pct_comp, pct_bs;
    uint64_t *out;
    size_t out_member, out_comp, out_bs;
    uint64_t *m0[2] = {nullptr, nullptr};  // optional: member 0's two components go here instead (entry stride m0_bs[k]) -- giant
    size_t m0_bs[2] = {0, 0};              // step j = 0 opens the outer accumulators with a copy (:425-433), which this saves
    int nlimbs, mod0;  // limbs [0, nlimbs) of the part; mod0 = modulus record of limb 0 in the ring's table
    double terms;      // (host, accounting) diagonals the group multiplies
};
hipError_t launch_diag_mac_group(const RingDev &r, const DiagMacGroupArgs &a, int batch, hipStream_t s);

// The baby steps ("leaves") of a polynomial evaluation, a GROUP of them in one pass over the power basis
// (circuits/common/polynomial/polynomial_evaluator.go:254-359, mapping == nil: Add(res, c_0), then MulThenAdd(X[k], c_k, res) for
// k = deg ... 1): per member g of the group, ciphertext component c and limb l <= level[g],
//   out[g][c] = CRed(c_{g,0} [c == 0] + CRed(MRedLazy128(sum_k MForm(c_{g,k}) * X_k[c]))),
// the canonical words the reference's sequence leaves (every step of it ends fully reduced): exact 128-bit accumulation, the
// high word reduced after every term as in the diag kernels, so the sum is exact for any term count with moduli below 2^62.
// A scalar is a pair of residues per limb, the first for coefficients [0, N/2) and the second for [N/2, N) (what
// he_double_rns_scalarop takes; BGV passes the same residue twice).  Each X_k word is loaded once per group (non-temporal).
// Scalar table (device, built once per polynomial): member g's words start at tab + off[g]; scalar k of it is
//   [2 k + h][limb] with stride L words, h = the half; k = 0 is the constant as a plain residue, k >= 1 in Montgomery form.
// present[g]: bit k = member g has term k (bit 0: the constant).  xlevel[k - 1]: the highest limb at which some member reads X_k
// (the caller has checked that X_k has it).  A null x[k - 1][c] / out[g][c]: the power / the member has no such component.
constexpr int kPolyLeafMaxTerms = 31;  // non-constant terms of one leaf the kernel admits: 2^logSplit - 1 with logSplit <= 5
constexpr int kPolyLeafGroupMax = 4;
struct PolyLeafGroupArgs {
    const uint64_t *tab;
    int L, n_powers, members, ncomp;  // ncomp: 2, or 3 when some power is of degree 2 (lazy)
    uint32_t off[kPolyLeafGroupMax], present[kPolyLeafGroupMax];
    int level[kPolyLeafGroupMax];
    int xlevel[kPolyLeafMaxTerms];
    const uint64_t *x[kPolyLeafMaxTerms][3];
    size_t x_bs[kPolyLeafMaxTerms][3];
    uint64_t *out[kPolyLeafGroupMax][3];
    size_t out_bs[kPolyLeafGroupMax][3];
    int nlimbs;  // 1 + the highest level of the group
};
hipError_t launch_poly_leaf_group(const RingDev &r, const PolyLeafGroupArgs &a, int batch, hipStream_t s);

// Fused "forward row NTT + key multiply-accumulate" for limbs below 2^47 (double-precision path): one workgroup
// owns (row, limb, batch entry) and loops over the beta digits; every non-own digit's row is transformed in LDS and
// multiplied by the two key rows straight out of LDS, the own digit's row is read from the NTT-domain input, the two
// accumulators stay in registers and are written once.  The transformed decomposition never goes to HBM.
struct NttMacArgs {
    int beta, nlimbs;
    uint8_t dec_limb[kMaxLimbs], key_limb[kMaxLimbs], out_limb[kMaxLimbs], out_view[kMaxLimbs], mod[kMaxLimbs];
    size_t dec_dstride, key_kstride, key_dstride;
    int own_alpha, own_nq;
    int dec_f64;     // the decomposed (non-own) words are doubles (launch_modup_fused f64_raw)
    int own_reduce;  // the own-digit words are caller-supplied (any uint64): reduce them before the conversion to double
    int q_out_f64;   // Q-limb accumulators are written as IEEE doubles (exact integers, |x| < q) for the f64 ModDown epilogue
};
// ModDown epilogue fused into the NTT + MAC kernel (production row sizes; every limb of the launch a Q limb of the
// double-precision class): after the key inner product of a (limb, row) the kernel transforms that row of the basis-extended P
// part of BOTH accumulators -- `ext`, [2 * batch] entries as launch_modup_fused left them, component c of entry b at c * batch + b
// -- and writes
//     out_c = [w_c +] MRed(NTT(ext_c) + 2q - acc_c, s[limb])        (the last op of ModDownQPtoQNTT, as NttEpilogue)
// against the accumulator still in registers: the Q accumulators are never written or read back, and the forward-row + epilogue
// launch over these limbs disappears.  tensor: w_c is formed from the product's inputs (NttEpilogue::tensor).
// sp[i] = IMForm(s[i]) and tsp[i] = IMForm(IMForm(ts[i])) as doubles, by launch limb.  out0Q / out1Q of the launch are unused.
struct NttMacEpilogue {
    View ext;
    bool ext_f64 = false;  // the extension's words are doubles (launch_modup_fused f64_raw)
    View out0, out1;
    bool has_w0 = false, has_w1 = false;
    View w0, w1;
    bool tensor = false;
    View ta0, ta1, tb0, tb1;
    double sp[kMaxLimbs], tsp[kMaxLimbs];
    uint32_t scatter_ginv = 0;  // as NttEpilogue::scatter_ginv
};
bool ntt_mac_epilogue_supported(int logN);
struct KsScatter;
// giant (optional, without an epilogue, production row sizes): the accumulators leave through KsScatter's giant-step stores
hipError_t launch_ntt_mac_f64(const RingDev &r, const NttMacArgs &a, View dec, View own, const double *keyd, View out0Q,
                              View out0P, View out1Q, View out1P, int batch, hipStream_t s, const NttMacEpilogue *epi = nullptr,
                              const KsScatter *giant = nullptr);
bool ntt_mac_giant_supported(int logN);
// keyd = (double)IMForm(key) for the limbs of class 2 (plain residues < 2^47), 0 elsewhere.  With rows of 4096 / 8192 coefficients
// (ntt_row_bits >= 12) each row is permuted for the NTT + MAC kernel: position k T + t (T = row / 16) holds coefficient 16 t + k.
hipError_t launch_key_to_f64(const RingDev &r, const uint64_t *key, double *keyd, int nblocks, const uint8_t *limb_mod_host,
                             int nlimbs, hipStream_t s);

// ---- BFV quantize (schemes/bgv/evaluator.go:1050-1071, coefficient domain) -----------------------------
// The middle of the reference's quantize(level, levelQMul, c2Q1, c2Q2) per coefficient, with no HBM round trip between its four
// steps: ModDownQPtoP (the extension Q -> QMul of cQ as ModUpQtoP does it, then z_j = MRed(e_j + 2 m_j - cM_j, m_j - c_j)),
// ModUpPtoQ of z (centred by QMul / 2) and MulScalar by t.  `r`: the combined table of a basis extender Q | QMul (Q moduli first);
// up: GenModUpConstants(Q[:nq], QMul), down: GenModUpConstants(QMul[:nm], Q), both resident.  cQ: nq limbs, cM: nm limbs,
// canonical coefficient-domain words; out: nq limbs, canonical; out may be cQ (a thread reads all its words before it writes).
// No entry tables.
struct BfvQuantizeArgs {
    int nq, nm;                  // limbs of Q (level + 1) and of QMul (levelQMul + 1), each 1..32
    int mod_m0;                  // modulus record of QMul limb 0 in r.mc (the Q limbs are records 0..nq-1)
    uint64_t q_half_q[32];       // (Q / 2) mod q_i: added before the first reconstruction
    uint64_t q_half_m[32];       // (Q / 2) mod m_j: subtracted after it
    uint64_t div_s[32];          // m_j - modDownConstantsQtoP[level][j]
    uint64_t m_half_m[32];       // (QMul / 2) mod m_j
    uint64_t m_half_q[32];       // (QMul / 2) mod q_i
    uint64_t t_mont[32];         // MForm(t mod q_i)
};
hipError_t launch_bfv_quantize(const RingDev &r, const ModUpDev &up, const ModUpDev &down, const BfvQuantizeArgs &a, View cQ, View cM,
                               View out, int batch, hipStream_t s);

// ---- CKKS encoder (schemes/ckks/encoder.go, double-precision path; include/hering_ckks_encoder.h) -------------------------
// The special FFT / iFFT of ckks_vector_ops.go:18-76 over n = 2^logn complex128 per batch entry, butterfly for butterfly (one IEEE
// operation per written operation, no fused multiply-add, complex product (ac - bd, ad + bc)).  Up to 2^kCkksFftLdsLog values one
// workgroup per entry runs every stage in LDS (two arrays of doubles: 2^13 x 16 B = 128 KiB of the 160 KiB a workgroup may
// declare); above, one launch per outer stage over global memory and the LDS kernel on blocks of 2^kCkksFftLdsLog for the rest.
constexpr int kCkksFftLdsLog = 13;
constexpr int kCkksDecodeMaxLimbs = 32;  // limbs rns_to_f64_kernel reconstructs (multi-word integer in registers)
struct CkksFftDev {
    const double *roots;  // [M + 1][2]: GetRootsComplex128(M) (utils.go:53-77), or the caller's table
    const uint32_t *rot;  // [M / 4]: 5^j mod M
    int logM;             // M = NthRoot of the ring
};
// Where the quantiser (SingleFloat64ToFixedPointCRT, utils.go:171-234, placed as Complex128ToFixedPointCRT :130-153 places it)
// writes: limbs 0..nQ-1 of outQ with the modulus records mcQ[0..nQ) (device), optionally limbs 0..nP-1 of outP; coefficient c of
// [re(slots) | im(slots)] lands at position c << log_gap, every other word of the polynomial is 0.  No entry tables.
struct CkksQuantArgs {
    const ModConst *mcQ = nullptr, *mcP = nullptr;
    View outQ{nullptr, 0}, outP{nullptr, 0};
    int nQ = 0, nP = 0;
    int logN = 0, log_gap = 0;
    int standard = 1;  // 0: conjugate-invariant ring (imaginary parts discarded)
    double scale = 0.0;
};
// in -> out ([batch][n][2] doubles, out != in).  logn > kCkksFftLdsLog: `work` is needed -- inverse: work == in, whose contents the
// outer stages overwrite; forward: unused (the outer stages run in place on out).  quant (inverse, logn <= kCkksFftLdsLog only):
// the values are not stored; the kernel's last step quantises them from LDS into the polynomial(s), zeros included -- ONE launch.
hipError_t launch_ckks_fft(const CkksFftDev &t, const double *in, double *out, double *work, int logn, int batch, bool inverse,
                           const CkksQuantArgs *quant, hipStream_t s);
// the quantiser as a launch of its own: src = [batch][n][2] slot values (direct = false), or [batch][N] real coefficients, already
// zero-padded (direct = true: Float64ToFixedPointCRT, utils.go:156-168)
hipError_t launch_f64_to_rns(const double *src, int logn, bool direct, const CkksQuantArgs &q, int batch, hipStream_t s);
// RNS -> float64 of the coefficients Decode needs (encoder.go:823-1116): batched -- slot i gets (coefficient i << log_gap,
// coefficient N/2 + (i << log_gap)) / scale as [batch][slots][2] (conjugate-invariant: the imaginary part is -real of slot
// slots - i, 0 for i = 0, :965-970); not batched -- every coefficient, [batch][N] reals ([N][2] with cplx).  g / Qw: device tables
// of host_math's build_garner_table / the level's modulus (Q little-endian in kCkksDecodeMaxLimbs words, then Q >> 1).
struct CkksDecodeArgs {
    int nl = 0;  // limbs (level + 1), 1..kCkksDecodeMaxLimbs
    int log_slots = 0, log_gap = 0, batched = 1, standard = 1, cplx = 1;
    double scale = 1.0;
    const uint64_t *g = nullptr, *Qw = nullptr;
};
hipError_t launch_rns_to_f64(const RingDev &r, const CkksDecodeArgs &a, View src, double *dst, int batch, hipStream_t s);

// ---- BGV / BFV encoder (schemes/bgv/encoder.go; include/hering_bgv_encoder.h) ------------------------------------------------
// ringT is a ring of one modulus T and degree n_t = 2^logNT; mcT: its resident modulus record.  No entry tables anywhere here.
constexpr int kBgvQ2TMaxLimbs = 32;  // the [32]uint64 of reconstructRNS (ring/basis_extension.go:550)
// Slots -> ring T (EncodeRingT :214-255 before its transform): dst[b][j] = reduce(values[b][inv[j]]) when inv[j] < n_values, else 0,
// for every j < n_t -- one thread per word of the polynomial, so the stores are contiguous and every word is written.  inv: the
// inverse of the index matrix (device, uint32 [n_t]); null: the identity (the coefficient encoding).  values: device, [batch][n_values].
// is_signed: the sign / BRedAdd sequence of :237-244 in wrapping arithmetic; a negative multiple of T gives 0.
hipError_t launch_bgv_slots_to_t(const ModConst *mcT, const uint32_t *inv, const uint64_t *values, size_t n_values, bool is_signed, View dst,
                                 int logNT, int batch, hipStream_t s);
// Ring T -> slots (DecodeRingT :349-368 after its transform): values[b][i] = src[b][perm[i]] for i < n_t, centred
// (v >= T >> 1 -> v - T) when is_signed.  perm: the index matrix (device, uint32 [n_t]); null: the identity.
hipError_t launch_bgv_t_to_slots(const ModConst *mcT, const uint32_t *perm, View src, bool is_signed, uint64_t *values, int logNT, int batch,
                                 hipStream_t s);
// Ring T -> RNS fan-out (RingT2Q :378-407 with the MulScalar of EncodeRingT :259 in front and MForm behind): word c of src (read
// once) becomes c' = MRed(c, scale_t) modulo T (scale_t = MForm_T(scale); 0: c' = c), and coefficient j << log_gap of limb i of
// outQ (nQ limbs, records mcQ[0..nQ)) is MRed(c', cQ[i]) modulo q_i, canonical for ANY 64-bit c' -- cQ[i] = MForm(k_i) for the
// factor k_i wanted (1, T^-1 mod q_i, times 2^64 for a Montgomery-form output).  The words between and after the strides are 0.
// outP (nP limbs, mcP, cP): the same from the same read; nP = 0: none.
struct BgvFanoutArgs {
    const ModConst *mcQ = nullptr, *mcP = nullptr;
    View outQ{nullptr, 0}, outP{nullptr, 0};
    int nQ = 0, nP = 0;
    int logN = 0, log_gap = 0;
    uint64_t scale_t = 0;
    uint64_t cQ[kMaxLimbs], cP[kMaxLimbs];
};
hipError_t launch_bgv_t_to_rns(const ModConst *mcT, View src, const BgvFanoutArgs &a, int batch, hipStream_t s);
// RNS -> ring T (RingQ2T :412-467, with the MulScalar of DecodeRingT :346 / Decode :496 behind it): one thread per coefficient j of
// ringT reads coefficient j << log_gap of the nl limbs of src (records r.mc[0..nl)) and writes dst[b][j], canonical modulo T.
//   pre[i] != 0 (scale_down): the word is first MRed(word, pre[i]), pre[i] = MForm(T mod q_i);
//   nl = 1: the level-0 lane (:447-465), word for word;
//   nl > 1, log_gap = 0: CRed(x_i + half_q[i]), reconstructRNS' float sum and multSum into T with `up` (GenModUpConstants(Q[:nl],
//   {T}) resident), minus half_t, as modup_kernel does them helper by helper; the result reduced to [0, T);
//   nl > 1, log_gap > 0: the Garner digits of rns_to_f64_kernel (g / Qw as in CkksDecodeArgs), x = sum d_i q_0 .. q_{i-1} compared with
//   Q >> 1; the word is sum MRed(d_i, prod_t[i]) - [x >= Q >> 1] q_mod_t modulo T, prod_t[i] = MForm_T(q_0 .. q_{i-1} mod T);
//   post != 0: the result times post * 2^-64 modulo T (post = MForm_T(scale^-1)).
struct BgvQ2TArgs {
    int nl = 0, log_gap = 0;
    uint64_t post = 0;
    uint64_t half_t = 0, q_mod_t = 0;
    const uint64_t *g = nullptr, *Qw = nullptr;
    uint64_t pre[kBgvQ2TMaxLimbs], half_q[kBgvQ2TMaxLimbs], prod_t[kBgvQ2TMaxLimbs];
};
hipError_t launch_bgv_rns_to_t(const RingDev &r, const ModConst *mcT, const ModUpDev &up, const BgvQ2TArgs &a, View src, View dst, int logNT,
                               int batch, hipStream_t s);

// ---- ring samplers (ring/sampler_uniform.go, sampler_gaussian.go, sampler_ternary.go; include/hering_sampler.h) ------------------
// The byte stream a sampler would have read from its PRNG is resident (`stream`, 8-byte aligned); a call parses it into `batch`
// polynomials, entry 0 first, each starting where the reference's next Read starts.  status: four device words, zeroed by the caller:
// [0] 0 done, 1 the stream ended first (nothing may be used), 2 the reference panics; [1] the bytes consumed in the reference's sense
// (chain launches); [2] non-zero: a word was rejected in the direct uniform launch (run the chain launch, which rewrites everything).
// UniformSampler.read (:44-99), `nparts` Reads per entry (2: the Q part and then the P part of a ringqp.Poly, ringqp/samplers.go:
// 47-55), part k into limbs 0..nl-1 of its polynomial.  chain = false: one thread per word, valid when no word is rejected,
// avail_words >= batch * sum roundup(nl_k N, 128); chain = true: one workgroup, any stream.
struct SamplerPart {
    const ModConst *mc;  // [nl]
    uint64_t *out;
    size_t out_bs;
    int nl;
};
hipError_t launch_sampler_uniform(const uint64_t *stream, size_t avail_words, const SamplerPart *parts, int nparts, int N, int batch,
                                  bool chain, uint64_t *status, hipStream_t s);
// GaussianSampler.read, float64 branch (:158-174): vals[b][i] = coeffInt << 1 | sign of sample i (bound <= 2^62).  tables: device,
// 128 words kn, 128 float32 wn, 128 float32 fn (host_math's gaussian_ziggurat_tables).  One workgroup.
hipError_t launch_sampler_gaussian(const uint64_t *stream, size_t avail_words, const uint32_t *tables, double sigma, double bound,
                                   uint64_t *vals, int N, int batch, uint64_t *status, hipStream_t s);
// TernarySampler.sampleProba (:130-196): vals[b][i] = the index into matrixValues.  half: the two-bit form of P = 0.5 (one thread
// per coefficient, avail_bytes >= batch N / 4, status not written); else the Knuth-Yao walk with the words x0 / x1 that
// computeMatrixTernary cuts its rows from (one workgroup).
hipError_t launch_sampler_ternary(const uint8_t *stream, size_t avail_bytes, bool half, uint64_t x0, uint64_t x1, uint64_t *vals, int N,
                                  int batch, uint64_t *status, hipStream_t s);
// vals into limbs 0..nl-1 of out: gaussian -- the words of :172, then CRed(a + w) with add, then MForm with mont (:177-179);
// else lut1[j] / lut2[j] = matrixValues[j][1] / [2] (host arrays of nl words), then CRed(a + w) with add
hipError_t launch_sampler_expand(const ModConst *mc, const uint64_t *vals, bool gaussian, bool add, bool mont, const uint64_t *lut1,
                                 const uint64_t *lut2, View out, int N, int nl, int batch, hipStream_t s);

// ---- key generation (core/rlwe/keygenerator.go:287-330, gadgetciphertext.go:172-241; include/hering_keygen.h) -----------------
// A key as Evk::rows() views it: R rows of two components, component c of row r at key + (2 r + c) blk, each nq + np limbs of N
// words; limb y has the modulus record mc[mod[y]].  G: a device table [R][nq] -- MForm(P 2^(j pw2) mod q_y) on the Q limbs of the
// row's own digit and 0 elsewhere (the factor is never 0 modulo a prime q_y); null: no gadget term.  No entry tables.
struct EvkRowsArgs {
    uint64_t *key = nullptr;
    const uint64_t *c1 = nullptr;  // launch_evk_finish: where component 1 is read, laid out as key (key itself, or the CRP of a share)
    size_t blk = 0;
    int N = 0, rows = 0, nq = 0, np = 0;
    const ModConst *mc = nullptr;
    uint8_t mod[kMaxLimbs];
    const uint64_t *skOutQ = nullptr, *skOutP = nullptr;  // nq / np limbs, NTT and Montgomery (launch_evk_finish)
    const uint64_t *pt = nullptr;                         // nq limbs, NTT and Montgomery: skIn / the plaintext; null with G null
    const uint64_t *G = nullptr;
    int comp = 0;                                         // launch_gadget_add: the component that receives the term
};
// encryptZeroSkFromC1QP (encryptor.go:420-425) and the gadget term over every row, in place: component 0 holds NTT(e), canonical,
// component 1 of c1 the uniform c1;  c0 = CRed(MForm(c0) + q - MRed(c1, skOut)) [then CRed(c0 + MRed(pt, G))].  One launch.
hipError_t launch_evk_finish(const EvkRowsArgs &a, hipStream_t s);
// the gadget term alone: key[r][comp] = CRed(key[r][comp] + MRed(pt, G[r][y])) on the Q limbs where G is not 0
hipError_t launch_gadget_add(const EvkRowsArgs &a, hipStream_t s);

// ---- multiparty shares (multiparty/keygen_evk.go:186-215, keygen_relin.go:237-254; include/hering_multiparty.h) ----------------
// out[r][c] = CRed(a[r][c] + b[r][c]) for the components c < ncomp of every row of three keys of one shape (EvkRowsArgs's layout):
// ring.Add's single conditional subtraction, so words in [q, 2q) of lazy shares come out as the reference's.  out may be a or b.
struct GadgetAggArgs {
    const uint64_t *a = nullptr, *b = nullptr;
    uint64_t *out = nullptr;
    size_t blk = 0;
    int N = 0, rows = 0, ncomp = 1, nl = 0;
    const ModConst *mc = nullptr;
    uint8_t mod[kMaxLimbs];
};
hipError_t launch_gadget_aggregate(const GadgetAggArgs &a, hipStream_t s);
// GenRelinearizationKey (keygen_relin.go:261-276): out[r][0] = MForm(a[r][0]) (the aggregated round-two share, words in [0, 2q)),
// out[r][1] = MForm(b[r][1]) (the aggregated round-one share).  out may be a or b.  ncomp is not read.
hipError_t launch_rlk_finalize(const GadgetAggArgs &a, hipStream_t s);

// The two rounds of RelinearizationKeyGenProtocol after their draws (keygen_relin.go:133-183, :211-233), over every row at once, in
// place on the share: grid and layout as EvkRowsArgs.  sk = (skQ, skP) and the ephemeral key u = (uQ, uP): nq / np limbs, NTT and
// Montgomery.
//   round one: share[r][0], share[r][1] hold NTT(e0), NTT(e1), canonical; in: the CRP a in component 1.  G: [rows][nq], P 2^(j pw2)
//              mod q_y -- NOT in Montgomery form -- on the Q limbs of the row's own digit, 0 elsewhere, so that MRed(sk, G) is
//              IMForm(P sk) 2^(j pw2).    share[r][0] = CRed(CRed(e0 + MRed(sk, G)) + q - MRed(u, a));  share[r][1] = CRed(e1 + MRed(sk, a))
//   round two: share[r][0] holds NTT(e), canonical; in: the aggregated round-one share (h0, h1), canonical.  The reference's lazy word
//              sequence:                share[r][0] = CRed(CRed(MRedLazy(h0, sk) + e) + MRed(CRed(u + q - sk), h1)), in [0, 2q)
struct RkgRowsArgs {
    uint64_t *share = nullptr;
    const uint64_t *in = nullptr;
    size_t blk = 0;
    int N = 0, rows = 0, nq = 0, np = 0;
    const ModConst *mc = nullptr;
    uint8_t mod[kMaxLimbs];
    const uint64_t *skQ = nullptr, *skP = nullptr, *uQ = nullptr, *uP = nullptr;
    const uint64_t *G = nullptr;  // round one
};
hipError_t launch_rkg_round_one(const RkgRowsArgs &a, hipStream_t s);
hipError_t launch_rkg_round_two(const RkgRowsArgs &a, hipStream_t s);

// ---- RGSW encryption (core/rgsw/encryptor.go; include/hering_rgsw_encryptor.h) ---------------------------------------------------
// A table of nkeys RGSW ciphertexts, each two separately allocated keys of the shape above: gadget ciphertext u of ciphertext k
// starts at keys[2 k + u] (a device table of base addresses).  Table row t = (k 2 + u) rows + r; e holds NTT(e) of every table row,
// canonical, [nkeys 2 rows][nq + np][N] (blk words apart); component 1 of every row holds the uniform c1 as drawn.  sel: device,
// [nkeys], the plaintext of ciphertext k among the entries of pts (pt_stride words apart, nq limbs, NTT and Montgomery), -1: none.
struct RgswTableArgs {
    uint64_t *const *keys = nullptr;
    const int32_t *sel = nullptr;
    const uint64_t *e = nullptr;
    size_t blk = 0;
    int N = 0, rows = 0, nkeys = 0, nq = 0, np = 0;
    const ModConst *mc = nullptr;
    uint8_t mod[kMaxLimbs];
    const uint64_t *skQ = nullptr, *skP = nullptr;  // nq / np limbs, NTT and Montgomery
    const uint64_t *pts = nullptr;                  // null: every sel is -1
    size_t pt_stride = 0;
    const uint64_t *G = nullptr;                    // [rows][nq], as EvkRowsArgs::G
};
// per word of table row t: c0 = CRed(MForm(e) + q - MRed(c1, sk)); with sel[k] >= 0 and G[r][y] != 0 the term MRed(pts[sel[k]], G) is
// added to c0 for u = 0 and to c1 for u = 1 (c0 from the c1 as drawn; then c1 + term is stored).  One launch; 2 nkeys rows <= 65535.
hipError_t launch_rgsw_table_finish(const RgswTableArgs &a, hipStream_t s);

// ---- ring-degree switches (core/rlwe/element.go:250-313, ring/operations.go:380) ----------------
// One launch over `batch` entries: entries z >= zsplit read in2 and write out2 (entry z - zsplit), so that both components of a
// ciphertext go in one launch (zsplit >= batch, or in2 / out2 null: in / out only).  n_small = the small degree (>= 16), the large
// one n_small << log_gap (log_gap >= 1).  Limb y of the launch reads limb tab.in_limb[y], writes tab.out_limb[y].  No entry tables.
struct RingSwitchIO {
    View in, out;
    View in2{nullptr, 0}, out2{nullptr, 0};
    int zsplit = -1;
};
// SwitchCiphertextRingDegreeNTT, large -> small: out[j] = gap^-1 sum_{s<gap} in[j gap + s] mod q[tab.mod[y]] (the large ring's
// modulus records), canonical; gapinv_mont[y] = MForm(gap^-1) (host array, tab.n words).  Inputs below 2^62.
hipError_t launch_ring_degree_fold_ntt(const RingDev &large, const LimbTab &tab, const uint64_t *gapinv_mont, RingSwitchIO io,
                                       int n_small, int log_gap, int batch, hipStream_t s);
// MapSmallDimensionToLargerDimensionNTT: out[j gap + s] = in[j]
hipError_t launch_ring_degree_replicate_ntt(const LimbTab &tab, RingSwitchIO io, int n_small, int log_gap, int batch, hipStream_t s);
// SwitchCiphertextRingDegree: down (up = false) out[w] = in[w gap]; up out[w gap] = in[w], the other words of out untouched
hipError_t launch_ring_degree_stride(const LimbTab &tab, RingSwitchIO io, int n_small, int log_gap, bool up, int batch, hipStream_t s);
// The CKKS bridge (ring/conjugate_invariant.go:3-44) between a standard polynomial of N = 2n words per limb and the compressed
// conjugate-invariant one of n (>= 16).  Fold: out[j] = CRed(in[N-1-j] + in[j], q[tab.mod[y]]) for j < n, the sum wrapping in 64
// bits (`moduli`: any ring with those modulus records); the index table of the Galois element 2N - 1 is j -> N - 1 - j.
hipError_t launch_ci_bridge_fold(const RingDev &moduli, const LimbTab &tab, RingSwitchIO io, int n, int batch, hipStream_t s);
// Unfold: out[j] = out[N-1-j] = in[j] for j < n
hipError_t launch_ci_bridge_unfold(const LimbTab &tab, RingSwitchIO io, int n, int batch, hipStream_t s);

// ---- ring packing (core/rlwe/ring_packing.go) -----------------------------------------------------
// Operands by ciphertext component: entries z < zsplit are component 0, the others component 1 (entry z - zsplit), so that both
// components go in one launch (zsplit < 0 or >= batch: component 0 only).  x / y are read, o / p written; y and p are optional
// where the launcher says so.  Limbs 0..nlimbs-1 of the ring's moduli, standard rings only.  No entry tables.
struct RingPackIO {
    View x[2] = {{nullptr, 0}, {nullptr, 0}}, y[2] = {{nullptr, 0}, {nullptr, 0}};
    View o[2] = {{nullptr, 0}, {nullptr, 0}}, p[2] = {{nullptr, 0}, {nullptr, 0}};
    int zsplit = -1;
};
// Split's ring map (:205-225), N -> N/2: o[j] = (x[2j] + x[2j+1]) / 2, p[j] = (x[2j] - x[2j+1]) RootsBackward[N/2 + j] / 2 (p optional)
hipError_t launch_ring_split(const RingDev &large, RingPackIO io, int nlimbs, int batch, hipStream_t s);
// Merge's ring map (:410-417), N/2 -> N: o[2j] = x[j] + w y[j], o[2j+1] = x[j] - w y[j], w = RootsForward[N/2 + j] (y optional:
// the replication of x)
hipError_t launch_ring_merge(const RingDev &large, RingPackIO io, int nlimbs, int batch, hipStream_t s);
// Expand's inner step (:528-559): o[e] = x[e] + y[e], o[e + m] = (x[e] - y[e]) XInvPow2NTT[k]; batch = entries of both components
hipError_t launch_expand_step(const RingDev &r, RingPackIO io, int k, int m, bool sum_only, int nlimbs, int batch, hipStream_t s);
// out = XPow2NTT[k] (div: XInvPow2NTT[k]) of GenXPow2NTT (:772-810), read off the resident twiddles
hipError_t launch_xpow2_fill(const RingDev &r, View out, int k, bool div, int nlimbs, int batch, hipStream_t s);
// Pack's inner step (:697-765) before (post = false, x = XPow2NTT[k]) and after the automorphism of T over `count` pairs; tab: a
// device array [4][count] of the addresses of (a0 | a1 | b0 | b1), 0 = absent; words: polynomial limbs moved, for the profile
hipError_t launch_pack_step(const RingDev &r, const uint64_t *tab, View t0, View t1, int k, bool post, int count, double words,
                            int nlimbs, hipStream_t s);

// ---- ciphertext tensor product (schemes/ckks/evaluator.go:807-820, schemes/bgv/evaluator.go:634-647)
// c0 = MRed(MRed(a0,s),b0), c2 = MRed(MRed(a1,s),b1), c1 = CRed(MRed(MRed(a0,s),b1) + MRed(MRed(a1,s),b0))
// with the per-limb scalar s = 2^128 mod q (CKKS: MForm) or t*2^128 mod q (BGV: tMontgomery).
hipError_t launch_tensor(const RingDev &r, const LimbTab &tab, const uint64_t *scalar, View a0, View a1, View b0, View b1,
                         View c0, View c1, View c2, int batch, hipStream_t s);

// ---- the CKKS evaluator's linear forms over a whole ciphertext (include/hering_ckks_evaluator.h) ----------------------------
// ONE launch for all components: a thread owns its pair of adjacent coefficients of EVERY component of the operation, reads every
// input word of them and only then writes, so any output may be any input (crossed components included) and an operand shared
// by the components -- the plaintext and its Montgomery form, the Montgomery form of a scalar -- is loaded or formed once.
// Limbs 0 .. nlimbs - 1 of every operand, identity limb map; every view may carry an entry table.  N >= 4: a pair never straddles
// N/2.  Forms (schemes/ckks/evaluator.go), with [r] = MRed(., r[limb]) where `scaled` says so, i over the components:
//   CT_ADD / CT_SUB (evaluateInPlace :221-408; scaled 1: x is multiplied first, 2: y): z_i = CRed([r] x_i +- [r] y_i) for
//     i < min(nx, ny); beyond it z_i = [r] x_i, or [r] y_i / q - [r] y_i (Ring.Neg's word, :153-156) when they come from y
//   CT_SCALAR_ADD / CT_SCALAR_SUB (:80-86, :171-177): z_0 = CRed(x_0 +- s), z_i = x_i for 0 < i < nx (nx = 1: no copies)
//   CT_SCALAR_MUL (:629-666): z_i = MRed(x_i, s)
//   CT_SCALAR_MUL_ADD (:928-975; scaled 1: the accumulator is multiplied first, :959-964): z_i = CRed([r] z_i + MRed(x_i, s))
//   CT_PT_MUL (:842-869): m = MRed(y_0, 2^128 mod q) once, z_i = MRed(x_i, m)
//   CT_PT_MUL_ADD (:1158-1170; scaled 1: :1087-1096): z_i = CRed([r] z_i + MRed(x_i, m))
// s: s[limb] for the coefficients [0, N/2), s2[limb] for [N/2, N); r, s, s2 of the multiplying forms are in Montgomery form.
enum CtLinForm { CT_ADD = 0, CT_SUB, CT_SCALAR_ADD, CT_SCALAR_SUB, CT_SCALAR_MUL, CT_SCALAR_MUL_ADD, CT_PT_MUL, CT_PT_MUL_ADD, CT_FORM_COUNT };
struct CtLinArgs {
    int form, scaled;
    int nx, ny, nz;      // components of x, of y (CT_PT_*: 1, the plaintext; the scalar forms: 0) and of z
    View x[3], y[3], z[3];
    int nlimbs;
    uint64_t r[kMaxLimbs], s[kMaxLimbs], s2[kMaxLimbs];
};
hipError_t launch_ct_lin(const RingDev &r, const CtLinArgs &a, int batch, hipStream_t s);
double ct_lin_passes(const CtLinArgs &a);  // limb-polynomials one launch reads and writes, per limb and batch entry

// The ciphertext product accumulated onto a ciphertext (mulRelinThenAdd, schemes/ckks/evaluator.go:1104-1155), one launch:
//   c0 = CRed([r] acc0 + T(a0, b0)), c1 = CRed([r] acc1 + CRed(T(a0, b1) + T(a1, b0))), T(x, y) = MRed(MRed(x, 2^128 mod q), y),
//   c2 = T(a1, b1) when acc2 is absent (the relinearizing form: c2 goes to scratch), else CRed([r] acc2 + T(a1, b1)).
// has_r: the accumulators are first multiplied by the integer whose Montgomery residues are r[limb] (:1087-1096).  c_i may be
// acc_i (that is the entry's only form); every view may carry an entry table.
struct TensorAddArgs {
    View a0, a1, b0, b1, acc0, acc1, acc2, c0, c1, c2;
    int nlimbs, has_r;
    uint64_t r[kMaxLimbs];
};
hipError_t launch_tensor_add(const RingDev &r, const TensorAddArgs &a, int batch, hipStream_t s);

// ---- per-kernel HIP-event profiling (diagnostics: bench.py's roofline leg) --------------------
enum KernelId {
    K_NTT_COLS_FWD = 0, K_NTT_ROWS_FWD, K_NTT_ROWS_INV, K_NTT_COLS_INV, K_EW, K_GATHER, K_AUTO_COEFF, K_INDEX,
    K_MODUP, K_CENTER, K_KS_INNER, K_TENSOR, K_PROBE, K_CI_FOLD, K_MASK_SPREAD, K_NTT_ROWS_FWD_F64, K_NTT_ROWS_INV_F64,
    K_NTT_MAC_F64, K_DIAG_MAC, K_RING_FOLD, K_RING_REPLICATE, K_RING_STRIDE, K_RING_SPLIT, K_RING_MERGE, K_EXPAND_STEP,
    K_PACK_PRE, K_PACK_POST, K_XPOW2_FILL, K_RGSW_FUSED, K_AUTO_FUSED, K_CI_BRIDGE_FOLD,
    K_CI_BRIDGE_UNFOLD, K_BFV_QUANTIZE, K_CKKS_FFT, K_CKKS_FFT_PASS, K_CKKS_IFFT_QUANT, K_F64_TO_RNS, K_RNS_TO_F64,
    K_BGV_SLOTS_TO_T, K_BGV_T_TO_SLOTS, K_BGV_T_TO_RNS, K_BGV_RNS_TO_T,
    K_SAMPLER_UNIFORM, K_SAMPLER_UNIFORM_CHAIN, K_SAMPLER_GAUSSIAN, K_SAMPLER_TERNARY_KY, K_SAMPLER_TERNARY_HALF, K_SAMPLER_EXPAND,
    K_EVK_FINISH, K_GADGET_ADD, K_RGSW_TABLE_FINISH, K_GADGET_AGGREGATE, K_RKG_ROUND_ONE, K_RKG_ROUND_TWO, K_RLK_FINALIZE,
    K_DIAG_MAC_GROUP, K_POLY_LEAF_GROUP, K_CT_LIN, K_TENSOR_ADD, K_COUNT
};
const char *kernel_name(int id);
void prof_begin(hipStream_t s);                                // start recording the launches enqueued on stream s
bool prof_active(hipStream_t s);                               // is stream s being recorded?
int prof_end(hipStream_t s, int *counts, float *total_ms, double *total_bytes = nullptr);  // stop, sync events, fill [K_COUNT] arrays

// throughput probe used by bench.py --microbench (not on the product path)
hipError_t launch_modmul_probe(uint64_t *buf, size_t n, int iters, uint64_t q, uint64_t qinv, hipStream_t s);
hipError_t launch_modmul_f64_probe(double *buf, size_t n, int iters, double q, hipStream_t s);

// arithmetic probe (he_debug_arith): the scalar primitives one by one; the numbering is HE_ARITH_* of include/hering_debug.h
enum ArithOp {
    ARITH_MRED_LAZY = 0, ARITH_MRED, ARITH_MRED_LAZY_W32, ARITH_MRED_LAZY_ASM, ARITH_MRED128_LAZY, ARITH_BRED_ADD_LAZY,
    ARITH_BRED_ADD, ARITH_BRED_LAZY, ARITH_BRED, ARITH_MFORM_LAZY, ARITH_MFORM, ARITH_IMFORM_LAZY, ARITH_IMFORM, ARITH_BFLY_FWD,
    ARITH_BFLY_FWD_ASM, ARITH_BFLY_FWD_NC, ARITH_BFLY_FWD_NC_ASM, ARITH_BFLY_INV, ARITH_BFLY_INV_ASM, ARITH_BFLY_INV_SCALED,
    ARITH_BFLY_INV_SCALED_ASM, ARITH_MODMUL_F64, ARITH_REDUCE_F64, ARITH_CANON_F64D, ARITH_CANON_F64, ARITH_U52_TO_F64,
    ARITH_F64_TO_U52, ARITH_HALVE, ARITH_AUTO_DEST, ARITH_COUNT
};
// a, b, c, o0, o1: device arrays of n words (b, c, o1 may be null where the op does not use them); mc: ONE resident record
hipError_t launch_arith_probe(const ModConst *mc, int op, size_t n, const uint64_t *a, const uint64_t *b, const uint64_t *c,
                              uint64_t *o0, uint64_t *o1, hipStream_t s);

}  // namespace he
