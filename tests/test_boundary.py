"""tests/boundary.py without a GPU: the prime searches, the chain builder's class and distance assertions over every chain the
`-m gpu` boundary tests build, the word sources, and the raw-doubles bound at the shapes those tests pin."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import boundary as Bd
from tests.helpers import rng_for


@pytest.mark.parametrize("logN", [12, 15, 17])
@pytest.mark.parametrize("bits", [47, 51, 58, 61])
def test_primes_below_and_above_are_the_nearest(logN, bits):
    step = 2 << logN
    below, above = Bd.primes_below(bits, logN + 1, 3), Bd.primes_above(bits, logN + 1, 2)
    assert below == sorted(below, reverse=True) and above == sorted(above) and len(set(below + above)) == 5
    assert all(q < (1 << bits) and q % step == 1 and O.IsPrime(q) for q in below)
    assert all(q >= (1 << bits) and q % step == 1 and O.IsPrime(q) for q in above)
    # nothing NTT-friendly and prime lies between them and the boundary, or between neighbours
    for lo, hi in ((below[2], 1 << bits), ((1 << bits) - step + 1, above[1])):
        q = lo + step
        while q < hi:
            assert (not O.IsPrime(q)) or q in below or q in above, q
            q += step


def test_modulus_class_thresholds():
    assert [Bd.modulus_class(q) for q in ((1 << 47) - 1, 1 << 47, (1 << 58) - 1, 1 << 58, (1 << 61) - 1)] == [0, 1, 1, 2, 2]
    with pytest.raises(ValueError):
        Bd.modulus_class(1 << 61)


@pytest.mark.parametrize("logN,alpha", [(12, 3), (12, 7), (12, 8), (15, 6), (15, 7), (16, 5), (16, 6), (17, 5)])
def test_key_switch_chains_sit_at_the_boundaries(logN, alpha):
    """the chains of tests/test_gpu_mac_boundary.py: classes, distances (asserted inside class_chain), Q and P disjoint, and
    every special prime of an integer class"""
    q, p = Bd.boundary_chains(logN, alpha)
    assert len(q) == alpha + 2 and len(p) == alpha and not set(q) & set(p)
    assert [Bd.modulus_class(m) for m in q] == ([1, 0, 0, 0, 2] + [0] * alpha)[: alpha + 2]
    assert all(Bd.modulus_class(m) >= 1 for m in p)
    d = [m for m in q if m < (1 << 47)]
    assert d == Bd.primes_below(47, logN + 1, len(d))


def test_rescale_chains_meet_every_class_pair():
    """[s47, s58, s47, s61, s47, s58^, s47]: going down the chain the dropped modulus takes each class, and a dropped modulus
    of the double-precision and of the Harvey class meets destinations of every class.  Its one prime of the correction-free
    class is dropped last, over a double-precision destination only; [s61, s58, s47, s58] adds the other two pairs."""
    seen = set()
    for logN, letters in ((13, "didhdId"), (16, "didhdId"), (13, "hidi")):
        q = Bd.class_chain(logN, letters)
        cls = [Bd.modulus_class(m) for m in q]
        if letters == "didhdId":
            assert cls == [0, 1, 0, 2, 0, 2, 0] and q[5] >= (1 << 58) and q[5] - (1 << 58) < (1 << (logN + 8))
            assert {cls[level] for level in range(1, len(q))} == {0, 1, 2}
        pairs = {(cls[i], cls[level]) for level in range(1, len(q)) for i in range(level)}  # (destination, dropped)
        if letters == "didhdId":
            assert pairs == {(a, b) for a in range(3) for b in (0, 2)} | {(0, 1)}
        seen |= pairs
    assert seen == {(a, b) for a in range(3) for b in range(3)}


@pytest.mark.parametrize("logN", [9, 10, 11, 12])
def test_class_chain_builds_at_the_small_rings_of_the_rgsw_edge_tests(logN):
    """every letter, twice over (a Q chain and a special prime of the same kind), with class_chain's own class and distance
    assertions; the 14-bit prime 12289 is NTT-friendly up to logN 11"""
    for letter in "dihDI":
        q = Bd.class_chain(logN, letter * 2)
        assert q[1:] == Bd.class_chain(logN, letter, skip={letter: 1})
        above = letter.isupper()
        assert all((m >= (1 << Bd._LETTERS[letter][0])) == above and m % (2 << logN) == 1 for m in q)
    assert (12289 % (2 << logN) == 1) == (logN <= 11) and O.IsPrime(12289)


def test_class_chain_rejects_a_prime_too_far_from_its_boundary():
    with pytest.raises(AssertionError):
        Bd.class_chain(17, "d" * 40)  # forty primes = 1 mod 2^18 below 2^47 span more than 2^27


def test_raw_bound_table():
    """(2 + 5 nsrc + 2 logN) p + nsrc 2^32 over 2^53 with the largest NTT-friendly prime below 2^47: the table of
    tests/test_gpu_mac_boundary.py, and which side of the predicate each shape is on (exact integers for the comparison)"""
    table = {(12, 3): 0.64, (12, 5): 0.80, (12, 6): 0.875, (12, 7): 0.953, (12, 8): 1.03, (15, 3): 0.73, (15, 5): 0.89,
             (15, 6): 0.969, (15, 7): 1.05, (16, 3): 0.77, (16, 5): 0.92, (16, 6): 1.00, (17, 3): 0.80, (17, 5): 0.953}
    raw = {(12, 7): True, (12, 8): False, (15, 6): True, (15, 7): False, (16, 5): True, (16, 6): False, (17, 5): True}
    for (logN, nsrc), frac in table.items():
        p = Bd.primes_below(47, logN + 1, 1)[0]
        assert abs(Bd.raw_bound_fraction(logN, nsrc, p) - frac) < 0.006, (logN, nsrc)
        if (logN, nsrc) in raw:
            assert ((2 + 5 * nsrc + 2 * logN) * p + (nsrc << 32) < (1 << 53)) == raw[logN, nsrc], (logN, nsrc)


def test_word_sources():
    rng, N, q = rng_for(4711), 8192, Bd.primes_below(47, 14, 1)[0]
    cases = Bd.worst_case_inputs(rng, q, N)
    assert len(cases) == len(Bd.WORST_CASE_KINDS) == 7
    assert all(int(c.max()) < 2 * q for c in cases) and all(int(c.max()) < q for c in (cases[0], cases[1], cases[3], cases[5]))
    assert int(cases[0].min()) == q - 1 and int(cases[4].min()) == 2 * q - 1
    assert int(cases[1][::2].min()) == q - 1 and not cases[1][1::2].any()
    assert int(cases[2][1::2].min()) == 2 * q - 1 and not cases[2][::2].any()
    assert int(cases[3][: N // 2].min()) == q - 1 and not cases[3][N // 2:].any()
    # the cycle walks through its kinds, one per call, all limbs of a call alike
    cyc = Bd.WordCycle(Bd.CANONICAL_KINDS, start=3)
    mods = [q, Bd.primes_below(58, 14, 1)[0]]
    x = [cyc(rng, mods, N) for _ in range(5)]
    assert x[0].shape == (2, N) and int(x[0].max()) < mods[1]  # "uniform"
    assert [int(v) for v in x[1][:, 0]] == [m - 1 for m in mods] and np.array_equal(x[1], x[1][:, :1].repeat(N, axis=1))  # "max"
    assert not x[2][:, 1::2].any() and not x[3][:, N // 2:].any()
    # sparse tensor inputs: exactly one word of 2^64 - 1 per 4096 coefficients, never at the same place in two operands
    ops = [Bd.sparse_wild(rng, mods, N, k) for k in range(4)]
    big = np.uint64(0xFFFFFFFFFFFFFFFF)
    for i in range(len(mods)):
        where = [np.flatnonzero(o[i] == big) for o in ops]
        assert all(len(w) == N // 4096 and [int(v) // 4096 for v in w] == list(range(N // 4096)) for w in where)
        assert len({int(v) for w in where for v in w}) == 4 * (N // 4096)
        assert all(int(np.delete(o[i], w).max()) < mods[i] for o, w in zip(ops, where))
    assert where[0][0] % 64 != where[0][1] % 64 or where[0][0] // 64 % 64 != where[0][1] // 64 % 64  # moves with the block
    for case in Bd.TENSOR_CASES:
        a0, a1, b0, b1 = Bd.tensor_inputs(case, rng, mods, N)
        assert a0.shape == a1.shape == b0.shape == b1.shape == (2, N)
        # every product of the tensor term inside MRed's domain x y < q 2^64; "wild" is the headline test's pattern, whose lazy
        # a1 against arbitrary words stays below 2q 2^64
        for i, m in enumerate(mods):
            for x_, y_ in ((a0, b0), (a0, b1), (a1, b0), (a1, b1)):
                lazy = case == "wild" and x_ is a1
                assert int((x_[i].astype(object) * y_[i].astype(object)).max()) < ((2 * m if lazy else m) << 64), (case, i)
