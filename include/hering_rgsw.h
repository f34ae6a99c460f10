/*
 * hering_rgsw.h -- the RGSW external product of core/rgsw/evaluator.go (libhering.so): RLWE x RGSW -> RLWE, the inner
 * operation of blind rotation, LUT evaluation and CMux trees.
 *
 * The same conventions as hering.h (which this header includes): 0 on success, <0 on error (HE_E*), he_last_error() for the
 * message; outputs are caller-allocated and come last; every entry files its work on the context's queue (coalescing, deferred
 * submission; queued calls are served one by one) and records under he_graph_begin / he_graph_end.
 *
 * An RGSW ciphertext is `Value [2]rlwe.GadgetCiphertext` (core/rgsw/elements.go:12) and is passed as two key handles
 * (he_evk_create / he_evk_create_base2) of the same evaluator, shape, BaseTwoDecomposition and window counts.
 *
 * Levels come from the RGSW ciphertext (op1.LevelQ(), op1.LevelP()): polynomials need at least levelQ + 1 limbs and limbs above
 * levelQ of the outputs keep their words.  Inputs and outputs are in the NTT domain; input words lie in [0, 2q), outputs are
 * canonical.  in and out have the same batch and one key serves the whole batch, except in the select form.
 *
 * Operand identity (checked before anything is filed; a rejected call changes nothing): out0 == in0 and / or out1 == in1 is
 * allowed (the reference's op0 == opOut) and gives the words of the out-of-place call; in0 == in1 is allowed; every other pair
 * among the four polynomials, out0 == out1 included, is HE_EINVAL.
 *
 * The three branches of the reference:
 *  - levelP >= 1 (externalProductInPlaceMultipleP, :206-280): RNS digits; out = ModDown(GadgetProductLazy(in0, rgsw0) +
 *    GadgetProductLazy(in1, rgsw1)), the sum taken mod q on canonical words.
 *  - levelP < 1 (externalProductInPlaceSinglePAndBitDecomp, :130-204): bit windows (INTT(in_k)[i] >> j pw2) & mask of every limb
 *    of both components, transformed into every Q (and P) limb, then ModDown (levelP == 0) or a copy (levelP == -1).  With
 *    BaseTwoDecomposition == 0 the mask is all ones (:147-149): ONE UNCENTRED window per limb, not the centred decomposition of
 *    rlwe's gadget product -- keys made with he_evk_create (one special prime, levelQ + 1 digits) take this form here.
 *    BaseTwoDecomposition == 0 without a special prime is HE_EINVAL: he_evk_create has no form without P.
 *  - levelQ == 0, levelP == -1, q < 2^29 (externalProduct32Bit, :84-128): plain 64-bit products key * NTTLazy(window) summed
 *    without reduction.  Where the sum cannot wrap, 2 D W (q - 1) < 2^64 with D windows per component and W = 6q - 2 the
 *    largest word of NTTLazy (ring/ntt.go:133), its output is the canonical value of the bit-window branch and is served as
 *    such; where the bound fails the reference's output is an artefact of the wrap and the call is HE_EINVAL.
 *
 * Routes.  The generic route serves every accepted shape on standard and conjugate-invariant rings through the gadget-product
 * cores, one sum of the accumulators and one ModDown.  Standard rings with levelP < 1, 9 <= logN <= 11, at most 8 Q limbs and
 * (2 (levelQ + 1) N + N + N / 16) * 8 <= 65536 bytes of LDS -- logN 9: up to 7 Q limbs, logN 10: up to 3, logN 11: one -- take
 * ONE launch that does the whole product of a batch entry in one workgroup, ModDown included.  HERING_NO_RGSW_FUSED=1 (read
 * once) sends he_rgsw_external_product down the generic route.  he_rgsw_external_product_select exists only inside the domain
 * of the one-launch kernel and is HE_EINVAL outside it.
 *
 * The helpers of core/rgsw/evaluator.go:283-356 (AddLazy, Reduce, MulByXPowAlphaMinusOne[ThenAdd]Lazy) run as element-wise
 * launches over the words of the keys, every (digit, component, limb) row, with the reference's lazy words; they are followed by
 * what he_evk_commit does, in stream order.  They are not queued and must not run while another thread uses the keys.
 *
 * Key words.  Keys as created (he_evk_create*) or committed (he_evk_commit) hold canonical words.  The lazy helpers leave words
 * at or above q on the device, and the library keeps a bound M with every key -- its words lie below M q in every limb: 1 as
 * created, committed or after HE_RGSW_REDUCE; out.M + in.M after HE_RGSW_ADD_LAZY; 2 after HE_RGSW_MUL_LAZY; out.M + 2 after
 * HE_RGSW_MUL_THEN_ADD_LAZY and after he_rgsw_key_add_plaintext_lazy (polynomial words lie in [0, 2q)).  M is kept up to 2^32;
 * a key that reaches it has no known bound and both products refuse it until it is reduced.  The two products take
 * such keys exactly where the reference's own arithmetic is exact with them, M the larger bound of the two gadget ciphertexts
 * (of any key of the set in the select form), on both routes and with the words of the reference:
 *  - bit-window branch (levelP < 1): every MRed(key, y) has y = NTTLazy(window) <= 6q - 2 (ring/ntt.go:133) and needs
 *    key y < q 2^64: served when M q < 2^64 and (M q - 1)(6q - 2) < q 2^64 for every modulus of the product (the Q limbs up to
 *    levelQ and the special prime), i.e. about M <= 2^64 / 6q: M <= 2 for q < 2^60, M = 1 only for a 61-bit prime;
 *  - branch M (levelP >= 1): every MRedLazy(key, y) has y < 2q: served when M q < 2^64 and (M q - 1)(2q - 1) < q 2^64;
 *  - 32-bit branch: the plain sum must not wrap: served when 2 D W (M q - 1) < 2^64 (D, W as above).
 * Outside these bounds the reference's words depend on how its Montgomery products leave their domain and the call is HE_EINVAL
 * before anything is filed: HE_RGSW_REDUCE the key first.
 */
#ifndef HERING_RGSW_H
#define HERING_RGSW_H

#include "hering.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rgsw.Evaluator.ExternalProduct (core/rgsw/evaluator.go:39): (out0,out1) = (<(in0,in1), rgsw[.][0]>, <(in0,in1), rgsw[.][1]>) / P */
int he_rgsw_external_product(he_handle eval, he_handle in0, he_handle in1,
                             he_handle rgsw0, he_handle rgsw1, he_handle out0, he_handle out1);
/* a table of n RGSW ciphertexts of one shape, resident on the device (BlindRotationEvaluationKeySet's keys); the set keeps its
 * keys alive */
int he_rgsw_keyset_create(he_handle eval, int n, const he_handle *rgsw0, const he_handle *rgsw1, he_handle *set);
int he_rgsw_keyset_destroy(he_handle set);
/* batch entry b is multiplied by key sel[b] of the set; sel[b] == -1: out[b] = in[b] (limbs 0..levelQ).  n_sel == batch.  The
 * selection is a scalar argument: read during the call, frozen in a captured graph.  The keys' addresses are resident with the
 * set; a call is the kernel's launch after one small launch per 896 entries that writes the selection into scratch. */
int he_rgsw_external_product_select(he_handle eval, he_handle in0, he_handle in1, he_handle set,
                                    const int32_t *sel, int n_sel, he_handle out0, he_handle out1);

/* operations of he_rgsw_key_op on ONE gadget ciphertext (an RGSW ciphertext takes two calls) */
enum { HE_RGSW_ADD_LAZY = 0,          /* AddLazy, *Ciphertext case (:308-316): out += in, no reduction */
       HE_RGSW_REDUCE,                /* Reduce (:323): out = in mod q, canonical */
       HE_RGSW_MUL_LAZY,              /* MulByXPowAlphaMinusOneLazy (:335): out = MulCoeffsMontgomeryLazy(in, x) */
       HE_RGSW_MUL_THEN_ADD_LAZY };   /* MulByXPowAlphaMinusOneThenAddLazy (:347): out += MulCoeffsMontgomeryLazy(in, x) */
/* in, out: key handles of one evaluator and shape (out may be in); xQ / xP: powXMinusOne (ringqp.Poly: one polynomial over the
 * Q moduli and one over the P moduli, batch 1, NTT + Montgomery), read by the two multiplications only (0 otherwise; xP is 0
 * for keys without a special prime) */
int he_rgsw_key_op(int op, he_handle in, he_handle xQ, he_handle xP, he_handle out);
/* AddLazy, *Plaintext case (:285-307): pt holds one polynomial per window j (batch entry j, Q limbs); it is added without
 * reduction to component 0 of rgsw0 and to component 1 of rgsw1, on the Q limbs of each digit's own range */
int he_rgsw_key_add_plaintext_lazy(he_handle pt, he_handle rgsw0, he_handle rgsw1);

#ifdef __cplusplus
}
#endif
#endif /* HERING_RGSW_H */
