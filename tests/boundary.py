"""Moduli at the boundaries of the three arithmetic classes, and the worst-case words that go with them (host side; shared by
the `-m gpu` boundary tests and checked without a GPU in tests/test_boundary.py).

The kernels choose their arithmetic by modulus size: double precision below 2^47, correction-free integer butterflies below
2^58, Harvey form up to 2^61 (the reference's own limit, ring/ntt.go:169).  Every exactness argument of the first two classes
is a magnitude bound in the modulus, so the primes that test it are the largest NTT-friendly ones below each threshold, and the
primes that test the dispatch are the smallest ones at or above it."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

CLASS_BITS = (47, 58, 61)  # double precision below 2^47, correction-free integer below 2^58, Harvey form below 2^61


def primes_below(bits: int, log_nth_root: int, count: int):
    """the `count` largest primes q < 2^bits with q = 1 mod 2^log_nth_root"""
    out, step = [], 1 << log_nth_root
    q = (1 << bits) - step + 1
    while len(out) < count:
        if O.IsPrime(q):
            out.append(q)
        q -= step
    return out


def primes_above(bits: int, log_nth_root: int, count: int):
    """the `count` smallest primes q >= 2^bits with q = 1 mod 2^log_nth_root"""
    out, step = [], 1 << log_nth_root
    q = (1 << bits) + 1
    while len(out) < count:
        if O.IsPrime(q):
            out.append(q)
        q += step
    return out


def modulus_class(q: int) -> int:
    """index into CLASS_BITS of the arithmetic a modulus gets"""
    for c, bits in enumerate(CLASS_BITS):
        if q < (1 << bits):
            return c
    raise ValueError(f"{q:#x} is not below 2^61")


# one letter per limb: lower case = the largest primes below the class threshold, upper case = the smallest primes at or above
# it (which belong to the next class)
_LETTERS = {"d": (47, False), "i": (58, False), "h": (61, False), "D": (47, True), "I": (58, True)}


def class_chain(logN: int, letters: str, skip=None):
    """A chain of distinct NTT-friendly primes (= 1 mod 2N) by class letters: 'd' / 'i' / 'h' take the largest primes below
    2^47 / 2^58 / 2^61 in turn (the k-th occurrence of a letter takes the k-th largest), 'D' / 'I' the smallest ones at or
    above 2^47 / 2^58.  `skip` (letter -> count) starts a letter's sequence further from the boundary, so that two chains over
    the same ring (Q and P) stay disjoint.

    Asserted here, for every prime: its class against the thresholds 2^47 / 2^58 / 2^61, and its distance to the boundary --
    below 2^(logN + 8) for the first prime of a kind, below 2^(logN + 10) for the k-th (eight primes = 1 mod 2^18 below 2^47
    span about 2^25)."""
    skip = dict(skip or {})
    need = {}
    for c in letters:
        need[c] = need.get(c, 0) + 1
    pools = {}
    for c, n in need.items():
        bits, above = _LETTERS[c]
        pools[c] = (primes_above if above else primes_below)(bits, logN + 1, n + skip.get(c, 0))
    taken = {c: skip.get(c, 0) for c in need}
    chain = []
    for c in letters:
        bits, above = _LETTERS[c]
        k = taken[c]
        taken[c] += 1
        q = pools[c][k]
        edge = 1 << bits
        assert q % (2 << logN) == 1 and O.IsPrime(q), (c, k, q)
        if above:
            assert edge <= q and modulus_class(q) == CLASS_BITS.index(bits) + 1, (c, k, q)
        else:
            assert q < edge and modulus_class(q) == CLASS_BITS.index(bits), (c, k, q)
            assert bits == CLASS_BITS[0] or q >= (1 << CLASS_BITS[CLASS_BITS.index(bits) - 1]), (c, k, q)
        assert abs(edge - q) < (1 << (logN + (8 if k == 0 else 10))), (c, k, q, abs(edge - q).bit_length())
        chain.append(q)
    assert len(set(chain)) == len(chain)
    return chain


def boundary_chains(logN: int, alpha: int):
    """(Q, P) of a key-switch shape at the boundaries: L = alpha + 2 limbs of Q, [s58, s47, s47, s47, s61, s47, ...], and alpha
    special primes that alternate the integer classes (below 2^58, below 2^61) -- none of the double-precision class"""
    q = class_chain(logN, ("idddhd" + "d" * 8)[: alpha + 2])
    p = class_chain(logN, ("ih" * 4)[:alpha], skip={"i": 1, "h": 1})
    return q, p


def raw_bound_fraction(logN: int, nsrc: int, max_small_modulus: int) -> float:
    """the raw-doubles handover's bound (2 + 5 nsrc + 2 logN) p + nsrc 2^32 as a fraction of 2^53: the basis extension leaves
    unreduced doubles to the double-precision row kernels while this is below 1"""
    return ((2 + 5 * nsrc + 2 * logN) * max_small_modulus + nsrc * (1 << 32)) / float(1 << 53)


# ---------------------------------------------------------------------------------------------------------------
# words
# ---------------------------------------------------------------------------------------------------------------
def word_row(kind: str, rng, q: int, N: int) -> np.ndarray:
    """one limb of N words of one of the worst-case kinds"""
    q = int(q)
    if kind == "max":
        return np.full(N, q - 1, dtype=np.uint64)
    if kind == "alt":
        x = np.zeros(N, dtype=np.uint64)
        x[::2] = q - 1
        return x
    if kind == "alt_lazy":
        x = np.zeros(N, dtype=np.uint64)
        x[1::2] = 2 * q - 1
        return x
    if kind == "half":
        x = np.zeros(N, dtype=np.uint64)
        x[: N // 2] = q - 1
        return x
    if kind == "max_lazy":
        return np.full(N, 2 * q - 1, dtype=np.uint64)
    if kind == "uniform":
        return rng.integers(0, q, size=N, dtype=np.uint64)
    if kind == "uniform_lazy":
        return rng.integers(0, 2 * q, size=N, dtype=np.uint64)
    raise ValueError(kind)


CANONICAL_KINDS = ("max", "alt", "half", "uniform")
WORST_CASE_KINDS = ("max", "alt", "alt_lazy", "half", "max_lazy", "uniform", "uniform_lazy")


def worst_case_inputs(rng, q, N):
    """worst cases inside the reference's input domain: canonical words and lazy words below 2q (ring/ntt.go:164-171 takes
    U, V in [0, 2q))"""
    return [word_row(kind, rng, q, N) for kind in WORST_CASE_KINDS]


class WordCycle:
    """A word source for whole polynomials: call k returns [limbs][N] words of kind kinds[k mod len(kinds)], so that the
    entries of a batch, and the polynomials drawn one after the other, walk through every kind."""

    def __init__(self, kinds, start: int = 0):
        self.kinds, self.k = tuple(kinds), start

    def __call__(self, rng, mods, N):
        kind = self.kinds[self.k % len(self.kinds)]
        self.k += 1
        return np.stack([word_row(kind, rng, m, N) for m in mods])


def wild_words(rng, shape):
    """arbitrary 64-bit words (any of them is a valid operand of MRed against a word below 2q)"""
    return rng.integers(0, 1 << 63, size=shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=shape, dtype=np.uint64)


def sparse_position(limb: int, operand: int, block: int) -> int:
    """where, inside block `block` of 4096 coefficients of limb `limb`, operand `operand` (0..3) of a sparse tensor input holds
    its one word of 2^64 - 1: different for the four operands of a limb (1031 k mod 4096 is non-zero for k = 1, 2, 3, so a
    product never meets two such words) and moving with the limb and the block"""
    return (17 + 61 * limb + 1031 * operand + 257 * block) % 4096


def sparse_wild(rng, mods, N, operand: int) -> np.ndarray:
    """canonical uniform words with exactly one word of 2^64 - 1 per 4096 coefficients (sparse_position): in a kernel that
    decides per wave whether to reduce its operands first, single waves take that branch with one large lane among small ones"""
    out = np.empty((len(mods), N), dtype=np.uint64)
    for i, m in enumerate(mods):
        out[i] = rng.integers(0, int(m), size=N, dtype=np.uint64)
        for blk in range(max(1, N // 4096)):
            out[i, (blk * 4096 + sparse_position(i, operand, blk)) % N] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return out


TENSOR_CASES = ("max", "uniform_lazy", "wild", "sparse")


def tensor_inputs(case: str, rng, mods, N):
    """(a0, a1, b0, b1) of one batch entry of a ciphertext product, [limbs][N] each.  Every product of the tensor term stays
    inside MRed's domain x y < q 2^64: "wild" is the operand pattern of
    test_full_size_mulrelin_aliasing_squaring_lazy_inputs (a0 canonical, a1 below 2q, b0 and b1 arbitrary 64-bit words)."""
    if case in ("max", "uniform_lazy"):
        return tuple(np.stack([word_row(case, rng, m, N) for m in mods]) for _ in range(4))
    if case == "wild":
        return (np.stack([word_row("uniform", rng, m, N) for m in mods]), np.stack([word_row("uniform_lazy", rng, m, N) for m in mods]),
                wild_words(rng, (len(mods), N)), wild_words(rng, (len(mods), N)))
    if case == "sparse":
        return tuple(sparse_wild(rng, mods, N, operand) for operand in range(4))
    raise ValueError(case)
