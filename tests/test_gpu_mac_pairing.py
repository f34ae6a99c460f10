"""The 4096-row NTT + key-MAC kernel (`ntt_mac_f64_dma_kernel<12, ...>`) through every instantiation, every word of every batch
entry against `oracle.Evaluator` (`-m gpu`).

The kernel takes the two extension rows of an item's fused ModDown epilogue as one pair of transforms per wave (the tensor
form: EPI + TEN); its other forms run one transform at a time.  What a work item does depends on how many foreign digits it
transforms (beta - 1 for a Q limb, whose own digit is the NTT-domain input itself; beta for a P limb), on where its own digit
sits, on the batch (work list shorter than the grid; XCD swizzle or not) and on the epilogue form.  The cases:

* chains with one special prime (alpha = 1) at every level 0..5: beta = 1..6, so the count of foreign transformed digits per
  item takes each of 0, 1, 2, 3, 4, 5 and the own digit is the first, a middle and the last one (logN = 12);
* a chain with two special primes, at the top level and below it (logN = 12 and 15): the last digit is short (one limb) and
  the own digit is first, middle and last;
* a chain whose second special prime is below 2^47 (logN = 12): P-limb items, beta foreign digits each, no fused epilogue
  (the P part depends on this kernel), and GadgetProduct takes the double-format accumulators;
* batches 1 and 9 everywhere, the ragged 255 at logN = 12 (1 and 9: fewer items than workgroups; 9 and 255: odd item counts, no
  XCD swizzle); tests/test_gpu_headline.py holds the headline shape itself at 9 / 128 / 255 / 256.

Instantiations reached (template arguments LOGB, QF64, EPI, SCAT, TEN):
  GadgetProductLazy                      <12, false>                       plain accumulators (Q and P limbs)
  GadgetProduct (f64-class special prime) <12, true>                        double-format Q accumulators, read by the fused ModDown
  GadgetProduct                          <12, false, true>                  epilogue without addend
  Relinearize, ApplyEvaluationKey        <12, false, true>                  epilogue with addend(s)
  BGVMulRelin, CKKSMulRelin              <12, false, true, false, true>     epilogue forming the tensor term: the PAIRED form
  Automorphism (logN = 15)               <12, false, true, true>            epilogue storing through the automorphism
  LinTransGiantStep                      <12, false, false, true>           giant step, overwriting and accumulating
Every call is made twice on the same handles (no state between launches).  The forms themselves are in
tests/keyswitch_forms.py; tests/test_gpu_mac_boundary.py runs them at the class-boundary primes on worst-case words."""
import pytest

from tests.gpu_common import ctx  # noqa: F401
from tests.keyswitch_forms import Env as _Env, key_switch_forms as _key_switch_forms

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B", [1, 9, 255])
def test_every_foreign_digit_count_one_special_prime(ctx, B):
    """alpha = 1, levels 0..5: beta = 1..6, foreign transformed digits per item 0..5, every form (logN = 12)"""
    e = _Env(ctx, 12, [45] * 6, [55], 9100 + B)
    for level in ((5, 2, 0) if B == 255 else range(6)):
        _key_switch_forms(e, level, B, automorphism=False)


@pytest.mark.parametrize("logN,B", [(12, 1), (12, 9), (12, 255), (15, 1), (15, 9)])
def test_short_last_digit_and_own_digit_position(ctx, logN, B):
    """alpha = 2, seven Q limbs of which six double-precision: digits (2, 2, 2, 1) at the top level, (2, 2, 1) two levels below --
    the last digit short, the own digit first, middle and last; logN = 15 adds the epilogue that stores through the
    automorphism (eight 4096-rows per limb)"""
    e = _Env(ctx, logN, [55] + [45] * 6, [55, 55], 9200 + logN + B)
    for level in (6, 4):
        _key_switch_forms(e, level, B, automorphism=logN == 15)


@pytest.mark.parametrize("B", [1, 9, 255])
def test_special_prime_below_2_47(ctx, B):
    """one of the two special primes is a double-precision limb: P-limb items (beta foreign digits, no own digit), no fused
    epilogue in the kernel; GadgetProduct and the MulRelin forms go through the double-format accumulators"""
    e = _Env(ctx, 12, [45] * 4 + [55], [55, 45], 9300 + B)
    for level in (4, 2):
        _key_switch_forms(e, level, B, automorphism=False)
