/*
 * hering_ckks_encoder.h -- ckks.Encoder on the device: Encode / Embed, Decode / DecodePublic and the special FFT / iFFT of the
 * reference's double-precision path, the one it takes when prec <= 53 (schemes/ckks/encoder.go: Encode :156, embedDouble :216-337,
 * decodePublic :497-760, IFFT / FFT :765-820, polyToComplexNoCRT :823, polyToComplexCRT :924, polyToFloatCRT :1033,
 * polyToFloatNoCRT :1119; schemes/ckks/ckks_vector_ops.go: SpecialFFTDouble / SpecialIFFTDouble :18-76 and their unrolled twins;
 * schemes/ckks/utils.go: GetRootsComplex128 :53, Complex128ToFixedPointCRT :130, Float64ToFixedPointCRT :156,
 * SingleFloat64ToFixedPointCRT :171; schemes/ckks/scaling.go:46 scaleDown; core/rlwe/utils.go:187 NTTSparseAndMontgomery)
 * (libhering.so).
 *
 * Out of scope: the big.Float / bignum.Complex paths (embedArbitrary, Special(I)FFTArbitrary, the []*big.Float and
 * []*bignum.Complex outputs), (encryption and decryption are hering_encryptor.h).
 *
 * The same conventions as hering.h (which this header includes): 0 on success, <0 on error (HE_E*), he_last_error() for the
 * message; outputs come last.  Host buffers are borrowed for the duration of the call; every entry that moves host data returns
 * with its device work finished.  Ordering with the submission queue and deferred mode is that of he_poly_upload /
 * he_poly_download: an encode runs after the queued writers of its output, a decode after those of its input.  None of these
 * entries can be captured in a graph (HE_EINVAL), as no host transfer can.
 *
 * Arithmetic contract.  Every result is bit-identical to the reference's formulas as a default amd64 Go build evaluates them: one
 * IEEE-754 round-to-nearest-even operation per written operation, no fused multiply-add, complex product (ac - bd, ad + bc), as a
 * function of the table of roots the encoder holds.  The butterflies of a stage touch disjoint pairs, so the plain and the unrolled
 * schedules of the reference (and the blocking of the kernels) give the same words.  The division of a complex value by
 * complex(x, 0) is two real divisions; it can differ from Go's in the sign of a zero result only.
 *   Values are float64, complex ones interleaved (re, im).  Slot vectors are [batch][slots], coefficient vectors [batch][N].
 *
 * Differences from the reference, deliberate:
 *   - non-finite inputs (NaN, +-Inf) of he_ckks_encode / he_ckks_encode_qp / he_ckks_fft / he_ckks_ifft are HE_EINVAL before
 *     anything is written (the reference converts them with undefined results);
 *   - the cosines of the built-in table of roots come from this host's libm; Go's math.Cos is a pure-Go routine whose words may
 *     differ in the last place.  A caller that needs Go's bits passes Go's table to he_ckks_encoder_create;
 *   - a batched, sparse (slots < max), coefficient-domain (is_ntt = 0) encode writes the polynomial in Y = X^gap: the coefficients
 *     at stride gap and zeros between them.  The reference's loop for that case (core/rlwe/utils.go:235-240) clears words it has
 *     not moved yet once gap >= 4;
 *   - a decode reduces the words of a coefficient-domain plaintext before it reconstructs (canonical input: no difference).
 */
#ifndef HERING_CKKS_ENCODER_H
#define HERING_CKKS_ENCODER_H

#include "hering.h"

#ifdef __cplusplus
extern "C" {
#endif

/* GetRootsComplex128(nth_root) (utils.go:53-77) on the host, no device needed: out = (nth_root + 1) complex128.
 * angle = 2 * 3.141592653589793 / float64(nth_root); cos(angle * float64(i)) for the first quarter only, every other word a copy
 * or a negation of those, as :60-74 write them; out[nth_root] = out[0].  nth_root: a power of two, 8 <= nth_root <= 2^22. */
int he_ckks_roots_host(uint64_t nth_root, double *out);

/* NewEncoder (encoder.go:78-135) with prec <= 53 over ringQ and, for he_ckks_encode_qp, ringP (0: none) -- rings of one context,
 * degree and type (HE_EINVAL otherwise).  M = NthRoot of ringQ (2N standard, 4N conjugate-invariant), rotGroup[j] = 5^j mod M.
 * roots: NULL for the built-in table (he_ckks_roots_host), or the caller's M + 1 complex128 (all finite: HE_EINVAL otherwise),
 * copied.  Everything below is a function of the table the encoder holds.  The handle keeps the rings alive. */
int he_ckks_encoder_create(he_handle ringQ, he_handle ringP, const double *roots, he_handle *out);
int he_ckks_encoder_destroy(he_handle enc);
/* the table the encoder holds: M + 1 complex128 */
int he_ckks_encoder_roots(he_handle enc, double *out);
/* out[0] = log2 M; out[1] = LogMaxDimensions.Cols = log2(M / 4); out[2] = the largest logn the one-workgroup transform takes (the
 * multi-pass route starts above it); out[3] = the largest number of limbs (level + 1) he_ckks_decode accepts */
int he_ckks_encoder_info(he_handle enc, int out[4]);

/* Encoder.FFT / Encoder.IFFT (:765-820) on `batch` vectors of n = 2^logn complex128, in place in the host buffer
 * values[batch][n].  0 <= logn <= LogMaxDimensions (HE_EINVAL); batch 1..65535.
 * forward: bit reversal, then stages of length 2, 4 .. n with twiddle roots[(rotGroup[j] & mask) << logGap];
 * inverse: stages n .. 2 with twiddle roots[(lenq - (rotGroup[j] & mask)) << logGap], the division by n, the bit reversal.
 * n <= 2^out[2] of he_ckks_encoder_info: one launch, one workgroup per vector; above: one launch per outer stage and one for the
 * rest. */
int he_ckks_fft(he_handle enc, int logn, int batch, double *values);
int he_ckks_ifft(he_handle enc, int logn, int batch, double *values);

/* Encoder.Encode (:156-189) of `batch` vectors into the polynomial outQ (`batch` entries, at least level + 1 limbs of ringQ),
 * limbs 0..level.  values[batch][n_values], complex128 when is_complex; a vector shorter than slots (N when not batched) is
 * zero-padded (:309-312).
 *   is_batched: Embed / embedDouble -- slots = 2^log_slots, 0 <= log_slots <= LogMaxDimensions, n_values <= slots; the imaginary
 *   parts are dropped on a conjugate-invariant ring before the transform (:242-246); IFFT; Complex128ToFixedPointCRT (real parts
 *   first, imaginary parts from coefficient `slots`, zeros after) at stride gap = MaxSlots / slots; then, as
 *   NTTSparseAndMontgomery, the NTT when is_ntt and MForm when is_montgomery.
 *   not batched: Float64ToFixedPointCRT of n_values <= N reals (is_complex: HE_EINVAL), then the NTT when is_ntt; log_slots and
 *   is_montgomery are not read (the reference applies no MForm there, :183-185).
 * The quantiser, per coefficient and modulus, word for word: value == 0 -> 0; v = |value scale| in float64;
 *   v >= 2^64: the integer is v (v + 0.5 rounds back to v at 53 bits), the word v mod q, or q - (v mod q) for a negative value (the
 *   word q when q | v);  otherwise c = uint64(v + 0.5): positive -- c when c <= 0x1fffffffffffffff (unreduced even when c >= q),
 *   else BRedAdd(c); negative -- q - BRedAdd(c) when c > q (q when q | c), else q - c.
 *   A product that is zero (scale 0, or an underflow) is such a c = 0: the word 0, or q for a negative value.  A negative scale is
 *   outside the reference's domain (its conversion to uint64 is undefined): every word of that call is 0.
 * Coefficient-domain outputs (is_ntt = 0) carry exactly these words.  NTT-domain outputs are the strict NTT of them: canonical,
 * and equal to the NTT of the reduced words.  With slots <= 2^out[2] the IFFT and the quantiser (zeros included) are ONE launch.
 * HE_EINVAL (nothing is written): level the ring lacks; log_slots out of range; n_values > slots (N); n_values = 0 or values
 * NULL; a non-finite value or scale; batch outside 1..65535 or not outQ's; outQ of another context or degree or too few limbs. */
int he_ckks_encode(he_handle enc, int level, int log_slots, double scale, int is_batched, int is_ntt, int is_montgomery,
                   const double *values, size_t n_values, int is_complex, int batch, he_handle outQ);
/* The ringqp.Poly arm of embedDouble (:321-328): one IFFT feeding outQ (limbs 0..level_q of ringQ) and outP (limbs 0..level_p of
 * ringP; level_p = -1: outP is not read).  Always batched.  HE_EINVAL also: the encoder has no ringP and level_p >= 0; outP is outQ. */
int he_ckks_encode_qp(he_handle enc, int level_q, int level_p, int log_slots, double scale, int is_ntt, int is_montgomery,
                      const double *values, size_t n_values, int is_complex, int batch, he_handle outQ, he_handle outP);

/* Encoder.DecodePublic (:199, :497-760) of the plaintext polynomial pt (limbs 0..level of ringQ, any batch B) into
 * values[B][slots] (is_batched) or values[B][N] (not batched), complex128 when is_complex, else float64 (the real parts).
 * pt is not changed.  is_ntt: the strict INTT into scratch first.  Then per needed coefficient (batched: i gap and N/2 + i gap;
 * not batched: all) the exact integer x mod Q_level, centred x >= Q >> 1 -> x - Q, rounded to nearest-even to float64 and divided
 * by scale (level 0: the same value as -float64(q - c) / float64(c)).  Conjugate-invariant: values[i] -= i real(values[slots - i])
 * for i >= 1 (:965-970).  Then the special FFT, and with logprec != 0 math.Round(x 2^logprec) / 2^logprec (half away from zero)
 * on the real and, for complex outputs, the imaginary parts (:536-550).  A plaintext that is not batched gets no FFT and no
 * rounding (:757-759).
 * HE_EINVAL: level the ring lacks or above out[3] - 1 of he_ckks_encoder_info (32 limbs); log_slots out of range; scale zero or
 * not finite; pt of another context or degree or too few limbs; more than 65535 entries. */
int he_ckks_decode(he_handle enc, int level, int log_slots, double scale, int is_batched, int is_ntt, double logprec, he_handle pt,
                   int is_complex, double *values);

#ifdef __cplusplus
}
#endif
#endif /* HERING_CKKS_ENCODER_H */
