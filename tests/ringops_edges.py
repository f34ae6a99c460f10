"""The rings, operand words, scalars, shifts and Galois elements of tests/test_gpu_ringops_edges.py (host side: no device is
needed to build them, and tests/test_ringops_host.py checks without one that each family has the property it is built for).

A family is, per modulus, three columns (x, y, z) of the same length: the operands of one word of a binary form (a unary form
reads x, a scalar form x and z).  `lay` spreads the columns over polynomials: tuple t of a family sits at every position
p = t mod n' of the stream of all rows, with n' odd, so that consecutive occurrences alternate between the even and the odd word
of a thread's 16-byte pair and walk through the rows."""
from __future__ import annotations

import functools

import numpy as np

from tests import boundary as Bd
from tests import ringops_ref as F
from tests.helpers import rng_for

U = np.uint64
M64 = (1 << 64) - 1
N_UNIFORM = 1 << 12


# ---------------------------------------------------------------------------------------------------------------
# moduli
# ---------------------------------------------------------------------------------------------------------------
MIXED = "hdIiD"  # largest below 2^61, largest below 2^47, smallest from 2^58, largest below 2^58, smallest from 2^47


@functools.lru_cache(None)
def mixed_chain(logN, with27=False, ci=False):
    """neighbouring limbs differ in size both ways; ci: moduli = 1 mod 4N"""
    lr = logN + (1 if ci else 0)
    q = Bd.class_chain(lr, MIXED)
    sizes = [m.bit_length() for m in q]
    assert sizes[0] > sizes[1] < sizes[2] > sizes[3] > sizes[4] and sizes[3] > sizes[4], sizes
    if with27:
        q = q + Bd.primes_below(27, lr + 1, 1)
        assert q[-1].bit_length() == 27
    return tuple(q)


@functools.lru_cache(None)
def chain64():
    """64 distinct primes = 1 mod 32 of all three classes, interleaved (kMaxLimbs limbs in one launch, logN 4)"""
    pools = [Bd.primes_below(61, 5, 22), Bd.primes_below(47, 5, 21), Bd.primes_below(58, 5, 21)]
    q = [pools[i % 3][i // 3] for i in range(64)]
    assert len(set(q)) == 64 and all(m % 32 == 1 for m in q) and {Bd.modulus_class(m) for m in q} == {0, 1, 2}
    return tuple(q)


Q97, Q12289 = 97, 12289


# ---------------------------------------------------------------------------------------------------------------
# operand words
# ---------------------------------------------------------------------------------------------------------------
def canonical_edges(q):
    return [0, 1, (q - 1) // 2, (q + 1) // 2, q - 2, q - 1]


def lazy_edges(q):
    return [q, q + 1, 2 * q - 1, 2 * q, 2 * q + 1, 4 * q - 1]


def word_edges(q):
    """the 64-bit edges; two words with the low half all zero, two with it all one"""
    return [(1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63, (1 << 64) - q, M64,
            0xFEDCBA9800000000, q << 32 & M64 & ~0xFFFFFFFF, 0x01234567FFFFFFFF, (q << 32 | 0xFFFFFFFF) & M64]


EDGE_VALUES = {"canonical": canonical_edges, "lazy": lazy_edges, "word64": word_edges}
EDGE_FAMILIES = tuple(EDGE_VALUES)
FAMILIES = EDGE_FAMILIES + ("cred", "wrap", "uniform", "wild")

CRED_FORMS = ("Add", "Sub", "MulCoeffsBarrettThenAdd", "MulCoeffsMontgomeryThenAdd", "MulCoeffsMontgomeryThenSub")
CRED_SCALAR_FORMS = ("AddScalar", "SubScalar", "MulScalarThenAdd", "MulScalarThenSub")
WRAP_FORMS = ("MulCoeffsBarrettThenAddLazy", "MulCoeffsMontgomeryThenAddLazy", "MulCoeffsMontgomeryLazyThenAddLazy",
              "MulCoeffsMontgomeryThenSubLazy", "MulCoeffsMontgomeryLazyThenSubLazy")
CRED_TARGETS = (-1, 0, 1)  # the sum the conditional subtraction tests, as q + d
WRAP_TARGETS = (-1, 0, 1)  # the accumulator's true sum, as 2^64 + d


def _cross(vals):
    """every (x, y) of the values, with z walking through them too"""
    n = len(vals)
    x = [vals[i] for i in range(n) for _ in range(n)]
    y = [vals[j] for _ in range(n) for j in range(n)]
    z = [vals[(i + 2 * j + 1) % n] for i in range(n) for j in range(n)]
    return x, y, z


def _pairs(q, rng, zero=True):
    """the (x, y) under a planted accumulator: a zero product, the largest one, and three uniform non-zero ones"""
    return ([(0, q - 1)] if zero else []) + [(q - 1, q - 1), (1, 1)] + [(int(rng.integers(1, q)), int(rng.integers(1, q))) for _ in range(3)]


def term(form, x, y, q):
    """what a ...Then... form adds to its accumulator: the form itself on z = 0 (the reference's arithmetic wraps)"""
    return F.BINARY[form](x, y, 0, F.K(q))


def cred_cols(form, q, rng, scalar=None):
    """operands whose final sum -- the argument of the form's CRed -- is q - 1, q and q + 1"""
    k = F.K(q)
    xs, ys, zs = [], [], []
    if form in ("Add", "Sub", "AddScalar", "SubScalar"):
        for d in CRED_TARGETS:
            for a in (0, 1, q - 1, (q - 1) // 2, M64):
                if form == "Add":  # x + y = q + d
                    xs.append(a), ys.append((q + d - a) & M64), zs.append(0)
                elif form == "Sub":  # x + q - y = q + d
                    xs.append(a), ys.append((a - d) & M64), zs.append(0)
                elif form == "AddScalar":  # x + s = q + d
                    xs.append((q + d - scalar) & M64), ys.append(0), zs.append(0)
                else:  # x + q - s = q + d
                    xs.append((d + scalar) & M64), ys.append(0), zs.append(0)
    else:
        for d in CRED_TARGETS:
            for x, y in _pairs(q, rng):
                if form in CRED_SCALAR_FORMS:
                    t = F.MRed(x, F.SCALAR[form][0](scalar, k), k)
                elif form == "MulCoeffsMontgomeryThenSub":
                    t = q - F.MRed(x, y, k)
                else:
                    t = term(form.replace("ThenAdd", ""), x, y, q)
                xs.append(x), ys.append(y), zs.append((q + d - t) & M64)
    return xs, ys, zs


def wrap_cols(form, q, rng):
    """operands whose accumulator's true sum is 2^64 - 1 (no wrap), 2^64 (wraps to 0) and 2^64 + 1 (wraps to 1); no zero product
    (a term of 0 cannot carry the accumulator over)"""
    xs, ys, zs = [], [], []
    pairs = []
    while len(pairs) < 5:  # a term below 2 cannot carry 2^64 - 1 ... 2^64 + 1 over from a 64-bit accumulator
        pairs += [p for p in _pairs(q, rng, zero=False) if term(form, p[0], p[1], q) >= 2]
    for d in WRAP_TARGETS:
        for x, y in pairs[:5]:
            xs.append(x), ys.append(y), zs.append(((1 << 64) + d - term(form, x, y, q)) & M64)
    return xs, ys, zs


def cols(family, q, seed, form=None, scalar=None, n_uniform=N_UNIFORM):
    """(x, y, z) uint64 columns of one family at one modulus, or None where the family does not exist for the form.  The
    length depends on the family (and n_uniform) alone, never on q."""
    rng = rng_for(seed)
    if family in EDGE_VALUES:
        c = _cross(EDGE_VALUES[family](q))
    elif family == "cred":
        if form not in CRED_FORMS + CRED_SCALAR_FORMS:
            return None
        c = cred_cols(form, q, rng, scalar)
    elif family == "wrap":
        if form not in WRAP_FORMS:
            return None
        c = wrap_cols(form, q, rng)
    elif family == "uniform":
        return tuple(rng.integers(0, q, size=n_uniform, dtype=U) for _ in range(3))
    elif family == "wild":
        return tuple(Bd.wild_words(rng, n_uniform) for _ in range(3))
    else:
        raise ValueError(family)
    return tuple(np.array(v, dtype=U) for v in c)


def poly_cols(family, mods, seed, form=None, scalar=None, n_uniform=N_UNIFORM):
    """the columns of every limb: three arrays [limbs][n]"""
    per = [cols(family, q, seed + 17 * i, form, scalar, n_uniform) for i, q in enumerate(mods)]
    if per[0] is None:
        return None
    return tuple(np.stack([p[c] for p in per]) for c in range(3))


def period(n):
    return n if n & 1 else n + 1


def lay(columns, N, B):
    """pages of (x, y, z), each [B][limbs][N]: the stream position p holds tuple (p mod n') -- index n, where n is even, is tuple
    0 again.  An edge family's stream is 2 n' long (every tuple at an even and at an odd position), a uniform one's n."""
    n = columns[0].shape[1]
    np_ = period(n)
    need = 2 * np_ if n < N_UNIFORM else n
    per_page = N * B
    pages = -(-need // per_page)
    idx = np.arange(pages * per_page) % np_
    idx[idx == n] = 0
    out = []
    for k in range(pages):
        sel = idx[k * per_page:(k + 1) * per_page].reshape(B, N)
        out.append(tuple(np.ascontiguousarray(np.transpose(c[:, sel], (1, 0, 2))) for c in columns))
    return out


def positions(n, N, B):
    """[pages][B][N] tuple index at every position of `lay`"""
    np_ = period(n)
    need = 2 * np_ if n < N_UNIFORM else n
    pages = -(-need // (N * B))
    idx = np.arange(pages * N * B) % np_
    idx[idx == n] = 0
    return idx.reshape(pages, B, N)


# ---------------------------------------------------------------------------------------------------------------
# scalars, shifts, Galois elements
# ---------------------------------------------------------------------------------------------------------------
def scalars(mods):
    q0 = mods[0]
    return [0, 1, q0 - 1, q0, q0 + 1, mods[-1], 2 * q0, 1 << 63, M64]


def bigint_scalars(mods):
    p = 1
    for q in mods:
        p *= q
    return [p, p + 1, p - 1, -1, -3 * mods[0], (1 << 300) + 987654321]


def rns_scalars(mods):
    """per-limb words of MulRNSScalarMontgomery: 0, q_i - 1, q_i, 2^64 - 1, rotated along the chain"""
    kinds = [lambda q: 0, lambda q: q - 1, lambda q: q, lambda q: M64]
    return [np.array([kinds[(i + r) % 4](q) for i, q in enumerate(mods)], dtype=U) for r in range(4)]


def double_scalars(mods):
    """(s0, s1) per-limb pairs of the double-scalar forms, s0 != s1 in every limb, from the single-scalar list"""
    s = scalars(mods)
    out = []
    for r in range(len(s)):
        s0 = [s[(r + i) % len(s)] for i in range(len(mods))]
        s1 = [s[(r + i + 1 + (i & 1)) % len(s)] for i in range(len(mods))]
        assert all(a != b for a, b in zip(s0, s1))
        out.append((np.array(s0, dtype=U), np.array(s1, dtype=U)))
    return out


def shifts(N):
    return [0, 1, N - 1, N, N + 1, 2 * N - 1, 2 * N, 2 * N + 7, -1, -N - 2, (1 << 31) - 1, -(1 << 31)]


def galois_elements(N):
    """odd only (an even one is not a permutation)"""
    return [1, 3, 5, N + 1, 2 * N - 1, pow(5, 77, 2 * N), 2 * N + 5, (1 << 63) + 5, M64]


def permutation_operand(mods, N, seed):
    """[limbs][N] for the permutations: zeros (under every sign case), canonical, lazy and 64-bit words, walking with an odd
    period so that each kind meets every destination class"""
    rng = rng_for(seed)
    out = np.empty((len(mods), N), dtype=U)
    for i, q in enumerate(mods):
        vals = [0, 0, 1, q - 1] + lazy_edges(q)[:3] + word_edges(q)[3:6] + [int(rng.integers(0, q))]
        assert len(vals) & 1
        out[i] = np.array([vals[(j + i) % len(vals)] for j in range(N)], dtype=U)
    return out
