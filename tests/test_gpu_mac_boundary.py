"""The ModDown epilogue inside the NTT + key-MAC kernel (`ntt_mac_f64_dma_kernel`, NttMacEpilogue: the EPI / TEN / SCAT forms)
at the class-boundary primes, on worst-case words, every word of every batch entry against `oracle.Evaluator` (`-m gpu`).

The epilogue runs inside the kernel only when no special prime is of the double-precision class (gadget_product_core), so here
every special prime is an integer-class one: P alternates the largest primes below 2^58 and below 2^61, and Q is
[s58, s47, s47, s47, s61, s47, ...] with the largest primes below 2^47 (tests/boundary.py: class_chain("idddhd...")).  Each
test first proves the path: no separate forward row launch of the double-precision limbs, and the epilogue's bytes charged to
ntt_mac_f64 -- a shape that fell back to the separate epilogue launch fails instead of passing on the other path.

With these primes the double-precision exactness arguments lose the factor of four that the 45-bit GenModuli primes leave
them ("34q + input < 2^53"; "|y| < q: x - y stays an exact integer below 2^53"), and the raw-doubles handover of the basis
extension (modup_f64_raw_ok: (2 + 5 nsrc + 2 logN) p + nsrc 2^32 < 2^53, nsrc = alpha) runs near its limit and on both sides
of it.  The bound as a fraction of 2^53 (tests/test_boundary.py holds the table):

  logN  alpha  L   row kernel, column stages   bound   extension output
  12    3      5   4096, none                  0.64    raw doubles
  12    7      9   4096, none                  0.953   raw doubles
  12    8      10  4096, none                  1.03    reduced words
  15    6      8   4096, three                 0.969   raw doubles
  15    7      9   4096, three                 1.05    reduced words
  16    5      7   8192, three                 0.92    raw doubles
  16    6      8   8192, three                 1.00    reduced words
  17    5      7   8192, four                  0.953   raw doubles (the tightest supported shape)

L = alpha + 2: at the top level the digits are (alpha, 2), one level below (alpha, 1); the own digit of a limb is the first
and the last one.

Words, per entry of the batch (tests/boundary.py):
* ciphertext polynomials: all q - 1, alternating 0 / q - 1, half, uniform; GadgetProduct's input also takes the lazy words
  2q - 1 and uniform [0, 2q) (the whole worst-case set, as tests/test_gpu_headline.py feeds that entry point).  The other
  entry points get canonical words: their ciphertext polynomials are the epilogue's addends, which it takes as canonical;
* keys: component 0 all q - 1 in every limb of Q and P ("max") or alternating 0 / q - 1 ("alt"), component 1 uniform;
* tensor inputs of the MulRelins: all q - 1; uniform [0, 2q); wild (the operand pattern of
  test_full_size_mulrelin_aliasing_squaring_lazy_inputs); sparse -- canonical words with one word of 2^64 - 1 per 4096
  coefficients, at a position of its own for each of a0, a1, b0, b1 and each limb, so that single waves take the tensor-input
  conversion's reduce-first branch (`cvtb`, decided by __any per wave) with one large lane among 63 small ones;
* LinTransGiantStep accumulators: arbitrary odd 64-bit words.
Every call is made twice on the same handles."""
import os

import pytest

from tests.boundary import CANONICAL_KINDS, WORST_CASE_KINDS, WordCycle, boundary_chains
from tests.gpu_common import ctx  # noqa: F401
from tests.keyswitch_forms import ALL_FORMS, T_PLAIN, Env, key_switch_forms

pytestmark = pytest.mark.gpu

SWITCH_FORMS = ("GadgetProductLazy", "GadgetProduct", "Relinearize", "ApplyEvaluationKey", "Automorphism", "LinTransGiantStep")
TENSOR_FORMS = ("BGVMulRelin", "CKKSMulRelin", "squaring")
LARGE_RING_FORMS = ("GadgetProduct", "Relinearize", "CKKSMulRelin", "Automorphism", "LinTransGiantStep")
assert set(SWITCH_FORMS) | set(TENSOR_FORMS) == set(ALL_FORMS)


def _env(ctx, logN, alpha, key, seed):
    q, p = boundary_chains(logN, alpha)
    e = Env(ctx, logN, seed=seed, qmods=q, pmods=p, key=key)
    assert all(m >= (1 << 47) for m in e.p) and e.beta == 2
    return e


def _assert_epilogue_runs_in_the_mac_kernel(ctx, e, level, B):
    """one GadgetProduct and one BGVMulRelin under the launch profile: the double-precision limbs have no forward row launch
    of their own, and ntt_mac_f64 is charged the epilogue's traffic (launch_ntt_mac_f64: beta digits in, two key rows per digit
    for the batch, two accumulators' worth of output, + the two extension rows, + the four inputs of the product)"""
    if any(k.startswith("HERING_NO_") and v not in ("", "0") for k, v in os.environ.items()):
        return  # a run of the suite with one of the fusions switched off: other launches, other bytes
    (c0, c1, d0, d1), (g0, g1, h0, h1) = e.polys(level, B, 4)
    o = e.outs(level, B)
    small_q = sum(m < (1 << 47) for m in e.q[: level + 1])
    beta = (level + 1 + len(e.p) - 1) // len(e.p)
    limb = e.N * 8
    ctx.prof_begin()
    e.gev.GadgetProduct(level, g0, e.gkey, o)
    prof = ctx.prof_end_bytes()
    assert "ntt_rows_fwd_f64" not in prof, sorted(prof)
    assert prof["ntt_mac_f64"][2] == ((beta + 2 + 2) * B + 2 * beta) * small_q * limb, ("GadgetProduct", prof["ntt_mac_f64"])
    ctx.prof_begin()
    e.gev.BGVMulRelin(level, T_PLAIN, [g0, g1], [h0, h1], e.gkey, o)
    prof = ctx.prof_end_bytes()
    assert "ntt_rows_fwd_f64" not in prof, sorted(prof)
    assert prof["ntt_mac_f64"][2] == ((beta + 2 + 6) * B + 2 * beta) * small_q * limb, ("BGVMulRelin", prof["ntt_mac_f64"])


def _run(ctx, logN, alpha, B, key, forms, levels, case):
    """`case` numbers the parametrisations of a shape: it moves the seed and the starting points of the word cycles, so that
    the parametrisations of a shape together walk through every kind of word and every tensor case"""
    e = _env(ctx, logN, alpha, key, 9400 + 16 * logN + alpha + 1000 * case)
    L = len(e.q)
    ct_words, gp_words = WordCycle(CANONICAL_KINDS, case), WordCycle(WORST_CASE_KINDS, 2 * case)
    for i, level in enumerate(levels):
        _assert_epilogue_runs_in_the_mac_kernel(ctx, e, L - 1 - level, B)
        key_switch_forms(e, L - 1 - level, B, automorphism=logN >= 15, forms=forms, ct_words=ct_words, gp_words=gp_words,
                         tensor_case0=case + i * B)


@pytest.mark.parametrize("key", ["max", "alt"])
@pytest.mark.parametrize("alpha,B", [(3, 1), (3, 9), (7, 4), (8, 4)])
def test_every_form_4096_rows_no_column_stage(ctx, alpha, B, key):
    """logN = 12: one 4096-row per limb.  alpha = 3 at batches 1 and 9; alpha = 7 hands raw doubles over at 0.953 of the
    bound, alpha = 8 is past it and hands reduced words over.  Every form, top level and one below."""
    _run(ctx, 12, alpha, B, key, ALL_FORMS, (0, 1), case=("max", "alt").index(key))


@pytest.mark.parametrize("forms", ["switch", "tensor"])
@pytest.mark.parametrize("key", ["max", "alt"])
@pytest.mark.parametrize("alpha", [6, 7])
def test_every_form_4096_rows_three_column_stages(ctx, alpha, key, forms):
    """logN = 15, the headline ring: alpha = 6 runs the paired tensor form on raw doubles at 0.969 of the bound, alpha = 7 on
    reduced words.  Every form (the key-switch forms and the tensor forms as two parametrisations), top level and one below."""
    case = 2 * ("max", "alt").index(key) + ("switch", "tensor").index(forms)
    _run(ctx, 15, alpha, 2, key, SWITCH_FORMS if forms == "switch" else TENSOR_FORMS, (0, 1), case)


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("key", ["max", "alt"])
@pytest.mark.parametrize("logN,alpha,B", [(16, 5, 2), (16, 6, 2), (17, 5, 1)])
def test_8192_rows(ctx, logN, alpha, B, key, level):
    """logN = 16 (three column stages; raw doubles at 0.92 with alpha = 5, reduced words with alpha = 6) and logN = 17 (four
    column stages; 0.953, the tightest shape the fused extension supports): GadgetProduct, Relinearize, CKKSMulRelin (the
    8192-row kernel's run-time tensor form), Automorphism and LinTransGiantStep, at the top level or one below."""
    _run(ctx, logN, alpha, B, key, LARGE_RING_FORMS, (level,), case=2 * ("max", "alt").index(key) + level)
