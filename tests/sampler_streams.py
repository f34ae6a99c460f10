"""The byte streams the sampler tests feed to the device and to the restatement (tests/sampler_ref.py): random ones, functions of
a seed and an offset alone, and crafted ones that force one exit of a sampler each.

The Gaussian streams carry a condition (tests/test_sampler_host.py::test_gaussian_streams_do_not_depend_on_exp_log): the device's
exp and log are not Go's, so a stream is used on the device only if the restatement returns the same words and the same consumption
with exp and log as they are, moved 4 ulps up and moved 4 ulps down.  A stream that fails is replaced by another seed, never
compared more loosely."""
from __future__ import annotations

import struct

from tests import sampler_ref as R


def cat_source(prefix: bytes, seed: int) -> R.Source:
    """the bytes of `prefix`, then the random stream of `seed`"""
    tail = R.seeded_source(seed)

    def gen(off, n):
        head = prefix[off:off + n]
        rest = n - len(head)
        return head + (tail.gen(max(off, len(prefix)) - len(prefix), rest) if rest else b"")
    return R.Source(gen)


# ---- Gaussian ---------------------------------------------------------------------------------------------------------------
SIGMA, BOUND = 3.2, 19.2  # the reference's default error distribution (core/rlwe/params.go: DefaultXe)
M53 = 0x1fffffffffffff


def _u32(ju: int) -> bytes:
    """a draw's first word: the four bytes read, then the four skipped (sampler_gaussian.go:208-213)"""
    return struct.pack("<II", ju, 0xdeadbeef)


def _f64(mantissa: int) -> bytes:
    """a randF64 word with the given 53 low bits; the 11 bits above are masked off by the sampler and set here"""
    return struct.pack("<Q", (0x7ff << 53) | (mantissa & M53))


def _wedge_j(i: int, frac: float) -> int:
    """a j of strip i (j & 0x7f = i) above kn[i]: the draw goes to the wedge test; frac in (0, 1) places it between kn[i] and 2^31"""
    lo, hi = int(R.KN[i]) >> 7, (1 << 31) >> 7
    j = ((lo + 1 + int((hi - lo - 2) * frac)) << 7) | i
    assert int(R.KN[i]) <= j < (1 << 31) and j & 0x7f == i
    return j


TAIL_J = 0x7fffff80  # strip 0, above kn[0] = 0x76ad2212: the tail of the base strip
assert TAIL_J & 0x7f == 0 and TAIL_J >= int(R.KN[0])


def crafted_gaussian_prefix() -> bytes:
    """Every exit of normFloat64 and of the bound test, word by word:
      words 0-1    c = 0 with sign 0, then with sign 1 (j = 0: the strip, x = 0)
      words 2-4    the tail, accepted at its first round (u1 close to 1: x small; u2 = 1/2)
      words 5-11   the tail: a round with a zero mantissa word that goes on (x = +Inf, y finite), a round of two zero words
                   (x = y = +Inf: out of the loop, norm = +Inf, rejected by the bound), the draw after it
      words 12-13  the wedge of strip 64, accepted (u = 0: the left-hand side is fn[64])
      words 14-16  the wedge of strip 64, rejected (u = 1: the left-hand side is fn[63]), and the draw after it
      words 17-126 strip draws
      words 127-128 a wedge draw whose second word is the first of the next 1024-byte buffer"""
    strip = _u32(5 << 7 | 3)  # j = 643 in strip 3, far below kn[3]
    w = [_u32(0), _u32(1 << 31),
         _u32(TAIL_J), _f64(M53 - 1000), _f64(M53 >> 1),
         _u32(TAIL_J | 1 << 31), _f64(0), _f64(12345), _f64(0), _f64(0), strip, strip,
         _u32(_wedge_j(64, 0.5)), _f64(0),
         _u32(_wedge_j(64, 0.5) | 1 << 31), _f64(M53), strip]
    w += [strip] * (127 - len(w))
    w += [_u32(_wedge_j(100, 0.3)), _f64(0)]
    assert len(w) == 129
    return b"".join(w)


class GaussCase:
    def __init__(self, name, make, logN, batch, sigma=SIGMA, bound=BOUND):
        self.name, self.make, self.logN, self.batch, self.sigma, self.bound = name, make, logN, batch, sigma, bound

    def source(self) -> R.Source:
        return self.make()

    def __repr__(self):
        return self.name


# every Gaussian stream a GPU test uses: (stream, the degree and the batch it is read at, the distribution)
GAUSS_CASES = [
    GaussCase("random-logN4", lambda: R.seeded_source(101), 4, 1),
    GaussCase("random-logN8-b3", lambda: R.seeded_source(102), 8, 3),
    GaussCase("random-logN10-b3", lambda: R.seeded_source(103), 10, 3),
    GaussCase("random-logN12", lambda: R.seeded_source(104), 12, 1),
    GaussCase("random-logN12-b3", lambda: R.seeded_source(105), 12, 3),
    GaussCase("bound-is-sigma-logN8-b3", lambda: R.seeded_source(106), 8, 3, SIGMA, SIGMA),
    GaussCase("crafted-logN8", lambda: cat_source(crafted_gaussian_prefix(), 107), 8, 1),
    GaussCase("crafted-logN6-b3", lambda: cat_source(crafted_gaussian_prefix(), 108), 6, 3),
    GaussCase("census-logN8", lambda: R.seeded_source(109), 8, 1),
    GaussCase("census-logN12-b3", lambda: R.seeded_source(110), 12, 3),
    GaussCase("sequence-logN8-b3", lambda: R.seeded_source(111), 8, 3),
]
GAUSS = {c.name: c for c in GAUSS_CASES}


# ---- ternary ----------------------------------------------------------------------------------------------------------------
# bits of a byte are read from the lowest (sampler_ternary.go:279).  With Ternary{P: 2/3} a walk goes on while its bits are 0.
KY_LONG_WALK = bytes([0, 0, 0, 0x40])   # 30 zero bits, then a one: a walk of 31 columns
KY_REFILL = bytes([0x00, 0x04] * 40)    # walks of 11 columns: 16 samples need more than the 16 bytes of the first buffer at N = 16
# matrix words no density gives (include/hering_sampler.h, he_debug_sampler_ternary_words): column 1 and columns 3..54 hold no one
# in either row, so a walk that enters column 1 with d = 1 restarts at the next bit, and a walk of ones runs out of columns
KY_WORDS_RESTART = (1 << 55, 1 << 53)
