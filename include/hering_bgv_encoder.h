/*
 * hering_bgv_encoder.h -- bgv.Encoder (the encoder of the integer schemes, BGV and BFV) on the device: Encode / Embed / EmbedScale,
 * Decode, EncodeRingT / DecodeRingT, RingT2Q / RingQ2T (schemes/bgv/encoder.go: NewEncoder :49-108, permuteMatrix :110-133,
 * Encode :143-200, EncodeRingT :203-262, EmbedScale :268-334, Embed :336, DecodeRingT :341-374, RingT2Q :378-407, RingQ2T :412-467,
 * Decode :470-526; the ring-T rule of bgv.NewParameters, schemes/bgv/params.go:120-123; ring/basis_extension.go ModUpExact
 * :282-308 / reconstructRNS / multSum :550-673; ring/ring.go PolyToBigintCentered :469-509, SetCoefficientsBigint :399-413)
 * (libhering.so).
 *
 * Out of scope: bgv.Evaluator's dispatch on []uint64 operands, the linear-transformation and polynomial drivers (encryption
 * and decryption are hering_encryptor.h), conjugate-invariant rings (bgv.NewParameters forces the standard type).
 *
 * The same conventions as hering.h (which this header includes): 0 on success, <0 on error (HE_E*), he_last_error() for the
 * message; outputs come last.  Host buffers are borrowed for the duration of the call; every entry returns with its device work
 * finished.  Ordering with the submission queue and deferred mode is that of he_poly_upload / he_poly_download: a call runs after
 * the calling thread's queued requests.  None of these entries can be captured in a graph (HE_EINVAL); an encode carries host data
 * into a polynomial, as an upload does, and cannot be part of a recorded window either.
 *
 * Values are uint64_t words; with is_signed they are the bit patterns of int64_t.  Host value arrays are [batch][n_values] on the
 * way in and [batch][slots] ([batch][N] when not batched) on the way out.  slots = N_T = 2^logN_T, the degree of ringT;
 * gap = N_Q / N_T.  A plaintext is a polynomial plus the metadata the reference keeps in rlwe.MetaData, passed as arguments.
 *
 * Reduction of the inputs.  A uint64 value v becomes BRedAdd(v, T) (ring.Reduce, :224): any 64-bit word is accepted.  An int64
 * value c follows :237-244 in wrapping 64-bit arithmetic: sign = c >> 63, |c| = c * (1 - 2 sign) (so INT64_MIN gives 2^63),
 * a = BRedAdd(|c|), the word a for sign = 0 and T - a for sign = 1.
 *
 * Differences from the reference, deliberate:
 *   - a negative multiple of T gives the word T in the reference (T - 0); the device writes 0.  No output can tell them apart:
 *     both pass through the strict INTT (batched) or a Montgomery product (not batched), which give the canonical word;
 *   - RingT2Q without scale_up copies the words of pT unreduced in the reference (:389), so a word at or above q_i (possible when
 *     T > q_i) stays there; the device writes c mod q_i, the canonical representative, in every case;
 *   - RingT2Q with scale_up on a polynomial of ringP multiplies by T^-1 mod p_j; the reference's :405 takes the moduli of ringQ for
 *     that polynomial too, which is not the inverse of T in ringP;
 *   - RingQ2T at level > 0 with gap 1 returns the canonical representative of the word the reference leaves lazy (multSum's word
 *     plus one conditional subtraction of SubScalar).  Decode is unaffected: the MulScalar that follows canonicalises there too;
 *   - the coefficient encoding (is_batched = 0) is accepted only when N_T = N_Q.  For N_T < N_Q the reference scales (:191),
 *     extends (:436) and centres (:496-518) only the first N_T of the N words it holds: those calls are HE_EINVAL here.
 */
#ifndef HERING_BGV_ENCODER_H
#define HERING_BGV_ENCODER_H

#include "hering.h"

#ifdef __cplusplus
extern "C" {
#endif

/* NewEncoder (encoder.go:49-108) over ringQ, ringP (0: none; needed by he_bgv_encode_qp and to_p only) and ringT, the ring of the
 * plaintext modulus.  HE_EINVAL unless: ringT has exactly one modulus T; all rings are of the standard type and of one context;
 * ringP has the degree of ringQ; logN_T = min(logN_Q, v2(T - 1) - 1) (params.go:120-123); T is coprime to every modulus of Q and P
 * (T equal to a q_i has no inverse modulo Q).  The handle keeps the rings alive.  It holds on the device permuteMatrix(logN_T)
 * (:110-133) and its inverse; on the host, per limb of Q and P, T^-1 mod q_i and T mod q_i; per level below 32 limbs the constants
 * of GenModUpConstants(moduli[:level + 1], {T}) (:62), Q_level >> 1 modulo every q_i and T (:63-64), and the Garner constants of
 * the exact reconstruction. */
int he_bgv_encoder_create(he_handle ringQ, he_handle ringP, he_handle ringT, he_handle *out);
int he_bgv_encoder_destroy(he_handle enc);
/* out[0] = logN_T; out[1] = log2 gap; out[2] = the largest number of limbs (level + 1) he_bgv_ring_q2t / he_bgv_decode accept: 32,
 * the [32]uint64 of the reference's reconstructRNS; out[3] = 0, reserved */
int he_bgv_encoder_info(he_handle enc, int out[4]);
/* the index matrix (permuteMatrix(logN_T), :110-133): N_T words */
int he_bgv_encoder_index(he_handle enc, uint64_t *out);

/* EncodeRingT (:203-262) into pT, a polynomial of ringT (one limb, degree N_T) of `batch` entries:
 * pT[perm[i]] = reduce(values[i]) for i < n_values, 0 for the other slots (:252-255), INTT, MulScalar(scale).  Every word of pT is
 * written.  HE_EINVAL (nothing is written): values NULL; n_values = 0 or above N_T; scale outside [1, T); batch outside 1..65535
 * or not pT's; pT of another context or degree. */
int he_bgv_encode_ring_t(he_handle enc, uint64_t scale, const uint64_t *values, size_t n_values, int is_signed, int batch, he_handle pT);
/* DecodeRingT (:341-374) of pT (ringT, any batch B up to 65535) into values[B][N_T]: MulScalar(scale^-1 mod T), NTT,
 * values[i] = word at perm[i]; is_signed: centred, value >= T >> 1 -> value - T (:363).  pT is not changed. */
int he_bgv_decode_ring_t(he_handle enc, uint64_t scale, he_handle pT, int is_signed, uint64_t *values);

/* RingT2Q (:378-407): coefficient j of pT (ringT) becomes coefficient j gap of limbs 0..level of pOut (ringQ, or ringP with
 * to_p), every other word of those limbs 0; scale_up: times T^-1 mod q_i.  One launch; the words are canonical. */
int he_bgv_ring_t2q(he_handle enc, int level, int scale_up, int to_p, he_handle pT, he_handle pOut);
/* RingQ2T (:412-467): limbs 0..level of pQ (ringQ, coefficient domain) into pT (ringT); scale_down: times T mod q_i first (:423).
 *   level 0: (c + (q_0 >> 1) mod q_0) mod T - (q_0 >> 1) mod T, of the coefficients j gap (:447-465);
 *   level > 0, gap 1: AddScalarBigint(Q / 2), ModUpExact, SubScalarBigint(Q / 2) (:434-436) -- the sequential float64 sum of
 *   reconstructRNS word for word, in limb order, one IEEE operation per written one, no fused multiply-add; canonical word;
 *   level > 0, gap > 1: PolyToBigintCentered at stride gap (x >= Q >> 1 -> x - Q), exact, then mod T (:438-440).
 * The two level > 0 branches differ where the float sum of the first lands within an ulp of an integer, as they do in the
 * reference: just below x = Q >> 1 (x + Q / 2 just below Q) the first gives the word of x - Q.  HE_EINVAL: more than 32 limbs. */
int he_bgv_ring_q2t(he_handle enc, int level, int scale_down, he_handle pQ, he_handle pT);

/* Encode (:143-200; scale_up = 1) and Embed (:336; scale_up = 0) of `batch` vectors into limbs 0..level of outQ (ringQ, `batch`
 * entries).
 *   is_batched: EmbedScale (:268-334) -- EncodeRingT, RingT2Q, then the NTT when is_ntt and MForm when is_montgomery.  MForm commutes
 *   with the strict NTT and both results are canonical, so the factor 2^64 is folded into the fan-out's constant.
 *   not batched (N_T = N_Q only): the values reduced as above, zero-padded, MulScalar(scale) modulo T, RingT2Q, the NTT when is_ntt;
 *   no MForm (:194-196), is_montgomery is not read.
 * scale must be in [1, T) (NewScaleModT has reduced it; 0 has no inverse).
 * HE_EINVAL (nothing is written): a level the ring lacks; n_values = 0 or above N_T; values NULL; scale outside [1, T); batch
 * outside 1..65535 or not outQ's; outQ of another context or degree or with too few limbs; not batched with N_T < N_Q. */
int he_bgv_encode(he_handle enc, int level, uint64_t scale, int is_batched, int is_ntt, int is_montgomery, int scale_up,
                  const uint64_t *values, size_t n_values, int is_signed, int batch, he_handle outQ);
/* The ringqp.Poly arm of EmbedScale (:280-311): one transform modulo T feeding outQ (limbs 0..level_q of ringQ) and outP (limbs
 * 0..level_p of ringP; level_p = -1: outP is not read).  Always batched.  HE_EINVAL also: level_p >= 0 without ringP; outP is outQ. */
int he_bgv_encode_qp(he_handle enc, int level_q, int level_p, uint64_t scale, int is_ntt, int is_montgomery, int scale_up,
                     const uint64_t *values, size_t n_values, int is_signed, int batch, he_handle outQ, he_handle outP);

/* Decode (:470-526) of the plaintext polynomial pt (limbs 0..level of ringQ, any batch B up to 65535) into values[B][N_T]:
 * is_ntt: the strict INTT into scratch first; RingQ2T with scale_down; then batched -- DecodeRingT; not batched (N_T = N_Q only)
 * -- MulScalar(scale^-1 mod T) and, with is_signed, the centring.  pt is not changed.
 * HE_EINVAL: a level the ring lacks or above 31; scale outside [1, T); values NULL; pt of another context or degree or with too few
 * limbs; more than 65535 entries; not batched with N_T < N_Q. */
int he_bgv_decode(he_handle enc, int level, uint64_t scale, int is_batched, int is_ntt, he_handle pt, int is_signed, uint64_t *values);

#ifdef __cplusplus
}
#endif
#endif /* HERING_BGV_ENCODER_H */
