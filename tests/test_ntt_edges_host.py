"""tests/ntt_edges.py without a GPU: every chain of the case tables builds at its class boundaries (class_chain asserts class and
distance), the floor primes are the encoder's plaintext moduli, and the oracle alone satisfies, on every input the `-m gpu` tests
of tests/test_gpu_ntt_edges.py send, the identities those tests lean on."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import boundary as Bd
from tests import ntt_edges as E


def test_floor_primes_are_the_smallest_ntt_friendly_ones():
    assert [E.floor_prime(lr) for lr in range(5, 17)] == [97, 193, 257, 257, 7681, 12289, 12289, 12289, 40961, 65537, 65537, 65537]
    for lr in range(5, 17):
        q, step = E.floor_prime(lr), 1 << lr
        assert q % step == 1 and O.IsPrime(q) and q < (1 << 47)
        assert not any(O.IsPrime(m) for m in range(step + 1, q, step))


@pytest.mark.parametrize("case", E.TRANSFORM_CASES, ids=E.case_id)
def test_transform_chains_build_at_the_boundaries(case):
    ci, logN = case
    lr = E.log_root(logN, ci)
    assert lr == logN + (2 if ci else 1) and 4 <= lr - 1 <= 15
    q = E.transform_chain(logN, ci)
    assert len(q) == 9 == len(set(q)) and all(m % (1 << lr) == 1 and O.IsPrime(m) for m in q)
    # d d D i i I h h floor: classes 0 0 1 1 1 2 2 2 0, so that every prefix of three or more limbs changes class
    assert [Bd.modulus_class(m) for m in q] == [0, 0, 1, 1, 1, 2, 2, 2, 0]
    assert q[:8] == Bd.class_chain(lr - 1, E.TRANSFORM_LETTERS) and q[8] == E.floor_prime(lr) and q[8] < (1 << 47)
    for level in (3, 6):
        assert len({Bd.modulus_class(m) for m in q[: level + 1]}) >= 2
    assert [Bd.modulus_class(m) for m in q[:4]] == [0, 0, 1, 1]  # AtLevel(3): d, d, D, i


def test_expected_dispatch_of_the_prefixes():
    assert set(E.DISPATCH_CASES) <= set(E.TRANSFORM_CASES)
    for ci, logN in E.DISPATCH_CASES:
        q = E.transform_chain(logN, ci)
        assert [E.expected_dispatch(q[: level + 1]) for level in (2, 5, 8)] == [(2, [1]), (2, [1, 2]), (3, [1, 2])]
        # the limb that decides each prefix sits right at its threshold
        assert (1 << 47) <= q[2] < (1 << 47) + (1 << (E.log_root(logN, ci) + 7)) and (1 << 58) <= q[5] < (1 << 58) + (1 << (E.log_root(logN, ci) + 7))


def test_remaining_chains_build():
    big = Bd.class_chain(E.BIG_LOGN, E.BIG_LETTERS)
    assert [Bd.modulus_class(m) for m in big] == [0, 1, 1, 2, 2] and len(set(big)) == 5
    for case in E.PAIRING_CASES:
        ci, logN, batch = case
        q = E.pairing_chain(logN, ci)
        assert len(set(q)) == 3 and all(Bd.modulus_class(m) == 0 and m % (1 << E.log_root(logN, ci)) == 1 for m in q)
        # just over the threshold of the pairing, or (logN 4, batch 1 and 2) far below it; odd, so that a workgroup is left with
        # a single entry
        wgs = E.pairing_workgroups(logN, batch)
        assert (E.PAIRING_THRESHOLD <= wgs < E.PAIRING_THRESHOLD + 8 and batch % 2 == 1) or (logN == 4 and batch in (1, 2))
        assert E.pairing_sample(batch) == sorted(set(E.pairing_sample(batch))) and E.pairing_sample(batch)[-1] == batch - 1
    assert sorted({c[1] for c in E.PAIRING_CASES if c[2] > 2 and not c[0]}) == [4, 5, 8, 11, 13]
    for case in E.RESCALE_CASES:
        ci, logN, letters = case
        q = E.rescale_chain(case)
        assert len(set(q)) == len(letters) and all(m % (1 << E.log_root(logN, ci)) == 1 for m in q)
        assert [Bd.modulus_class(m) for m in q] == [{"d": 0, "i": 1, "h": 2, "I": 2}[c] for c in letters]
    assert sorted({(c[0], c[1]) for c in E.RESCALE_CASES}) == [(False, 4), (False, 5), (False, 8), (False, 11), (False, 12), (True, 4), (True, 10)]
    assert len(E.RESCALE_CASES) == 14 and len(E.TRANSFORM_CASES) == 21


def _oracle_identities(o, mods, x, in_domain):
    """The three identities on one polynomial.  The reference's transforms take words below 2q (ring/ntt.go:164-171); the
    arbitrary 64-bit entries of the second batch are outside that domain -- the oracle's own NTT of them is not the NTT of
    their residues -- which is why the device, whose public entries reduce first, is compared with the oracle on Reduce(x).
    For those entries the identities are stated on Reduce(x), the polynomial the oracle is then given."""
    r = o.unop("Reduce", x)
    assert np.array_equal(r, E.reduce_words(x, mods))
    twoq = 2 * np.array(mods, dtype=np.uint64)[:, None]
    assert bool(np.all(x < twoq)) == in_domain
    arg = x if in_domain else r
    f = o.NTT(arg)
    assert np.array_equal(f, o.NTT(r))
    assert np.array_equal(o.INTT(f), r)
    assert np.array_equal(o.INTT(arg), o.INTT(r))
    assert np.array_equal(o.unop("Reduce", o.INTTLazy(arg)), o.INTT(arg))


@pytest.mark.parametrize("case", E.TRANSFORM_CASES + ["big"], ids=lambda c: c if c == "big" else E.case_id(c))
def test_oracle_identities_on_the_transform_inputs(case):
    mods, x1, x2, nspec = E.transform_inputs(case)
    ci, logN = (False, E.BIG_LOGN) if case == "big" else case
    o = O.Ring(1 << logN, mods, ci)
    kinds = E.BIG_KINDS if case == "big" else Bd.WORST_CASE_KINDS
    assert x1.shape == (len(kinds), len(mods), 1 << logN) and x2.shape == (nspec + 2, len(mods), 1 << logN)
    assert bool((x2[-1] == E.ALL_ONES).all()) and not bool((x1 == E.SENTINEL).any())
    for x in x1:
        _oracle_identities(o, mods, x, True)
    for b, x in enumerate(x2):
        _oracle_identities(o, mods, x, b < nspec)
        if b < nspec:  # the spectra are the oracle's NTT of the first two entries: canonical, and they invert to them
            assert np.array_equal(o.INTT(x), o.unop("Reduce", x1[b]))


@pytest.mark.parametrize("case", E.RESCALE_CASES, ids=E.rescale_id)
def test_oracle_identities_on_the_rescale_inputs(case):
    ci, logN, letters = case
    mods, polys = E.rescale_inputs(case)
    o = O.Ring(1 << logN, mods, ci)
    assert len(polys) >= 6 and len(polys) % E.RESCALE_BATCH == 0
    for x in polys:
        assert x.shape == (len(letters), 1 << logN)
        _oracle_identities(o, mods, x, True)
    if ci:
        # the NTT-domain rescale of a conjugate-invariant ring hands the LAZY words of the top limb's inverse to the other
        # moduli: the case its exact representative is about did occur
        assert E.lazy_top_words(o, polys) > 0


def test_pairing_inputs_cycle_through_the_worst_case_kinds():
    mods, x = E.pairing_inputs((False, 4, 2049))
    assert x.shape == (2049, 3, 16)
    for b in range(2049):
        kind = Bd.WORST_CASE_KINDS[b % 7]
        if "uniform" not in kind:
            assert np.array_equal(x[b], np.stack([Bd.word_row(kind, None, m, 16) for m in mods])), b
    assert bool(np.all(x < 2 * np.array(mods, dtype=np.uint64)[None, :, None]))
    assert E.pairing_sample(2049) == [0, 1, 2, 3, 1024, 2047, 2048] and E.pairing_sample(1) == [0] and E.pairing_sample(2) == [0, 1]
