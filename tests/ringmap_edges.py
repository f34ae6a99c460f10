"""The rings, operand words and shapes of tests/test_gpu_ringmap_edges.py (host side: no device is needed to build them, and
tests/test_ringmap_host.py checks without one that each family has the property it is built for).

A planted family is, per modulus, a list of tuples: the words one butterfly (split, merge, expand, pack) or one fold sum reads
together.  They are spread over the polynomials as tests/ringops_edges.py spreads its columns (`positions`: tuple t sits at every
unit p = t mod n' of the stream of all rows, n' odd), so that consecutive occurrences alternate between the two words of a thread's
16-byte pair and walk through the rows.  Where a conditional subtraction follows a product with a twiddle word (merge, pack pre), the
second operand is chosen AFTER the product at that position: t = MRed(o, w_j) first, then e = q + d - t when that is canonical.

A row family is a whole polynomial of one of tests/boundary.py's worst-case kinds; entry b of a batch takes the b-th next kind, moved by
b positions, so that the entries differ."""
from __future__ import annotations

import functools

import numpy as np

from tests import boundary as Bd
from tests import ringmap_ref as M
from tests import ringops_edges as E
from tests import ringops_ref as F
from tests.helpers import rng_for

U = np.uint64

# ---------------------------------------------------------------------------------------------------------------
# moduli
# ---------------------------------------------------------------------------------------------------------------
Q193, Q12289 = 193, 12289
RING_MAX_MODULI = 48  # he_ring_create refuses more


def mixed(logN_large, ci=False):
    """`h d I i D` at the LARGE degree (= 1 mod 4N on a conjugate-invariant ring): neighbouring limbs differ in size both ways"""
    return E.mixed_chain(logN_large, False, ci)


@functools.lru_cache(None)
def chain49():
    """49 distinct primes = 1 mod 64 of the three classes, interleaved: the first 48 are the most limbs a ring of N = 32 can have"""
    pools = [Bd.primes_below(61, 6, 17), Bd.primes_below(47, 6, 16), Bd.primes_below(58, 6, 16)]
    q = [pools[i % 3][i // 3] for i in range(RING_MAX_MODULI + 1)]
    assert len(set(q)) == len(q) and all(m % 64 == 1 for m in q)
    return tuple(q)


def chain48():
    return chain49()[:RING_MAX_MODULI]


def rings_for(N_large, ci=False):
    """name -> chain: the mixed chain, and the single primes 193 and 12289 where the degree allows them"""
    out = {"mixed": mixed(N_large.bit_length() - 1, ci)}
    for q in (Q193, Q12289):
        if (q - 1) % ((4 if ci else 2) * N_large) == 0:
            out[f"q{q}"] = (q,)
    return out


def levels(nq):
    """the top level, the one below, level 0"""
    return sorted({nq - 1, max(nq - 2, 0), 0}, reverse=True)


# ---------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------
# (n, gap) of the ring-degree maps: the smallest degree through each template of the fold (a partial workgroup), one workgroup, two
# and mid-grid, and the largest ratio
DEGREE_SHAPES = ((16, 2), (16, 4), (16, 8), (16, 16), (512, 2), (1024, 4), (2048, 8), (16, 256))
PACK_DEGREES = (32, 1024, 2048)  # split / merge / expand / pack / xpow2: 32 is the smallest he_ring_split_ntt takes
BATCH = 3


def table_indices(logN):
    """k = 0, 1, logN - 2, logN - 1 (at the last the twiddle index is 1)"""
    return sorted({0, 1, logN - 2, logN - 1})


# ---------------------------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------------------------
PLANTED = ("cred", "canonical")  # (cred first: a failure names the family built for the subtraction)
ROWS = ("max", "alt", "alt1", "half", "uniform")  # boundary.CANONICAL_KINDS, and `alt` shifted by one position
LAZY_ROWS = ("max_lazy", "alt_lazy", "uniform_lazy")  # words below 2q: the fold, the replicate and the strides only
LAZY_PLANTED = ("lazy_multiples",)  # the fold only
CANONICAL_FAMILIES = PLANTED + ROWS
FOLD_FAMILIES = PLANTED + LAZY_PLANTED + ROWS + LAZY_ROWS
COPY_FAMILIES = ROWS + LAZY_ROWS
TARGETS = (-1, 0, 1)  # the argument of a conditional subtraction, as q + d
POSITIONAL = ("merge", "pack_pre")  # the forms whose conditional subtractions follow a product with a twiddle word


def _rot(g, r):
    r %= len(g)
    return g[-r:] + g[:-r] if r else list(g)


def row_entry(kind, rng, q, N):
    if kind == "alt1":
        return np.roll(Bd.word_row("alt", rng, q, N), 1)
    return Bd.word_row(kind, rng, q, N)


def rows(kind, mods, N, B, seed):
    """[B][limbs][N]: entry 0 of the kind itself, entry b of the b-th next kind of its cycle, moved by b positions"""
    cyc = LAZY_ROWS if kind in LAZY_ROWS else ROWS
    k0 = cyc.index(kind)
    rng = rng_for(seed)
    return np.stack([np.stack([np.roll(row_entry(cyc[(k0 + b) % len(cyc)], rng, q, N), b) for q in mods]) for b in range(B)])


def addsub_cred(q):
    """(a, b): a + b = q - 1, q, q + 1; a + q - b = 1, q - 1, q, q + 1, 2q - 1"""
    h = (q - 1) // 2
    out = [(a, q + d - a) for d in TARGETS for a in (2, h, h + 1, q - 1)]
    out += [(0, q - 1), (q - 1, 0)]
    out += [(a, a) for a in (0, 1, h, q - 1)]
    out += [(a, a + 1) for a in (0, h, q - 2)] + [(a + 1, a) for a in (0, h, q - 2)]
    assert all(0 <= a < q and 0 <= b < q for a, b in out)
    return out


def pair_specs(form, family, q, rng):
    """the tuples of a two-operand form: ("pair", x, y), or for the positional forms ("sum" | "dif", o, d): the first operand is
    made at the position, after the product (realise)"""
    if family == "canonical":
        v = E.canonical_edges(q)
        return [("pair", x, y) for x in v for y in v]
    assert family == "cred", family
    if form not in POSITIONAL:
        return [("pair", a, b) for a, b in addsub_cred(q)]
    os_ = [1, q - 1, (q - 1) // 2, int(rng.integers(1, q)), int(rng.integers(1, q))]
    out = [(kind, o, d) for kind in ("sum", "dif") for d in TARGETS for o in os_]
    return out + [("sum", 0, -1), ("dif", 0, 0), ("dif", 0, 1)]  # a zero product


def realise(spec, q, w):
    """(first operand, second operand) of a tuple at a position whose twiddle word is w (Montgomery form)"""
    kind, o, d = spec
    if kind == "pair":
        return o, d
    t = F.MRed(o, w, F.K(q))
    e = q + d - t if kind == "sum" else t + d  # e + t = q + d; e + q - t = q + d
    if not 0 <= e < q:  # not canonical at this position: the neighbouring target
        e = q - 1 - t if kind == "sum" else t
    return e, o


def fold_groups(family, q, gap, rng):
    """the tuples of the fold: `gap` words that one output sums"""
    v = E.canonical_edges(q)
    T = gap // 4
    out = []
    if family == "canonical":
        for ix, x in enumerate(v):
            for iy, y in enumerate(v):
                g = [x, y] + [v[(ix + iy * s + s) % len(v)] for s in range(2, gap)]
                out.append(_rot(g, ix * len(v) + iy) if gap > 2 else g)
        return out
    h = (q - 1) // 2
    if family == "cred":
        if gap == 2:  # sums 0, q - 1, q, q + 1: the output of an exact multiple must be 0 and not q
            return [[0, 0], [1, q - 1], [q - 1, 1], [h, h + 1], [h + 1, h], [0, q - 1], [q - 1, 0], [h, h], [2, q - 1], [q - 1, 2], [h + 1, h + 1]]
        quads = [[q - 1] * k + [k + d] + [0] * (3 - k) for k in (1, 2, 3) for d in TARGETS]  # sums k q + d
        if gap == 4:
            return [_rot(g, i) for i, g in enumerate(quads)] + [[0, 0, 0, 0]]
        # the generic path: acc + BRedAdd(partial) = q + d across a loop trip (r1 after one trip, r2 = q + d - r1 from the next) ...
        n = 0
        for d in TARGETS:
            for r1 in (max(1, 1 + d), h, q - 2, q - 1):
                r2 = q + d - r1
                assert 0 <= r2 < q
                t0 = n % (T - 1)
                g = [0] * gap
                g[4 * t0:4 * t0 + 4] = _rot([q - 1, q - 1, (r1 + 2) % q, 0], n)  # = r1 mod q, through BRedAdd's own subtraction
                g[4 * t0 + 4:4 * t0 + 8] = _rot([r2, 0, 0, 0], n)
                out.append(g)
                n += 1
        for i, quad in enumerate(quads):  # ... and BRedAdd on k q + d inside one trip
            g = [0] * gap
            g[4 * (i % T):4 * (i % T) + 4] = _rot(quad, i)
            out.append(g)
        return out
    assert family == "lazy_multiples", family
    z = 2 * q - 1
    if gap == 2:
        return [[q, q], [z, 1], [1, z], [z, q + 1], [q + 1, z], [q, 0], [0, q], [z, z], [z, 0], [z, 2], [z, q], [z, q + 2]]
    quads = [[z, z, 2 + d, 0] for d in TARGETS] + [[z, z, q + 2 + d, 0] for d in TARGETS] + [[z, z, z, 3 + d] for d in TARGETS] + \
            [[z, z, z, q + 3 + d] for d in TARGETS] + [[z, z, z, z]]  # 4q, 5q, 6q, 7q (+ d), 8q - 4
    for i, quad in enumerate(quads):
        g = [0] * gap
        g[4 * (i % T):4 * (i % T) + 4] = _rot(quad, i)
        out.append(g)
    return out


def fold_inputs(family, mods, n, gap, B, seed):
    """pages of [B][limbs][n gap]"""
    if family in ROWS + LAZY_ROWS:
        return [rows(family, mods, n * gap, B, seed)]
    per = [np.array(fold_groups(family, q, gap, rng_for(seed + 17 * i)), dtype=U) for i, q in enumerate(mods)]
    pages = []
    for pg in E.positions(len(per[0]), n, B):
        pages.append(np.ascontiguousarray(np.stack([g[pg].reshape(B, n * gap) for g in per], axis=1)))
    return pages


def pair_inputs(form, family, mods, units, B, seed, tw=None):
    """pages of (x, y), each [B][limbs][units]; tw[limb][unit]: the twiddle word of each unit (the positional forms)"""
    if family in ROWS + LAZY_ROWS:
        return [(rows(family, mods, units, B, seed), rows(family, mods, units, B, seed + 1))]
    per = [pair_specs(form, family, q, rng_for(seed + 17 * i)) for i, q in enumerate(mods)]
    pages = []
    for pg in E.positions(len(per[0]), units, B):
        x, y = np.empty((B, len(mods), units), dtype=U), np.empty((B, len(mods), units), dtype=U)
        for i, q in enumerate(mods):
            if per[i][0][0] == "pair" and per[i][-1][0] == "pair":
                x[:, i], y[:, i] = np.array([s[1] for s in per[i]], dtype=U)[pg], np.array([s[2] for s in per[i]], dtype=U)[pg]
                continue
            for b in range(B):
                xy = [realise(per[i][t], q, tw[i][u]) for u, t in enumerate(pg[b].tolist())]
                x[b, i], y[b, i] = [p[0] for p in xy], [p[1] for p in xy]
        pages.append((x, y))
    return pages


def interleave(x, y):
    """[..][units] x 2 -> [..][2 units]: word 2j from x, word 2j + 1 from y"""
    out = np.empty(x.shape[:-1] + (2 * x.shape[-1],), dtype=U)
    out[..., 0::2], out[..., 1::2] = x, y
    return out


def split_inputs(family, mods, N, B, seed):
    """pages of [B][limbs][N]: butterfly j reads (in[2j], in[2j+1])"""
    if family in ROWS:
        return [rows(family, mods, N, B, seed)]
    return [interleave(x, y) for x, y in pair_inputs("split", family, mods, N // 2, B, seed)]


def merge_twiddles(N, mods):
    """w of butterfly j: XPow2NTT[0][2j] of the materialised table"""
    return [row[0::2].tolist() for row in M.tables(N, tuple(mods), False)[0]]


def pack_twiddles(N, mods, k):
    return [row.tolist() for row in M.tables(N, tuple(mods), False)[k]]


# ---------------------------------------------------------------------------------------------------------------
# what each family is built for, from the integer model (tests/test_ringmap_host.py asserts it)
# ---------------------------------------------------------------------------------------------------------------
def _near(s, v, q):
    """collect v as its distance to q where that is -1, 0, 1"""
    if abs(v - q) <= 1:
        s.add(v - q)


def fold_arguments(a, q, gap):
    """one limb [..][n gap] -> {"sum": multiples k of q met exactly by a plain sum (gaps 2, 4), "acc": q + d met by acc + r across a
    trip, "bred": q + d met by BRedAddLazy inside BRedAdd, "max": the largest plain four-word sum}"""
    k = F.K(q)
    out = {"sum": set(), "sum_near": set(), "acc": set(), "bred": set(), "max": 0}
    for g in np.asarray(a).reshape(-1, gap).tolist():
        if gap <= 4:
            s = sum(g)
            out["max"] = max(out["max"], s)
            if s % q == 0:
                out["sum"].add(s // q)
            if s % q in (1, q - 1):
                out["sum_near"].add(1 if s % q == 1 else -1)
            continue
        acc = 0
        for t in range(0, gap, 4):
            p = sum(g[t:t + 4])
            out["max"] = max(out["max"], p)
            assert p < 1 << 64
            lazy = F.BRedAddLazy(p, k)
            _near(out["bred"], lazy, q)
            if t:
                _near(out["acc"], acc + F.CRed(lazy, q), q)
            acc = F.CRed(acc + F.CRed(lazy, q), q)
    return out


def pair_arguments(form, x, y, q, tw=None):
    """one limb, x / y [..][units] (tw[unit] per unit of the LAST axis) -> {"sum": d met by the additive conditional subtraction,
    "dif": d met by the subtractive one, "dif_arg": the values of a + q - b among 1, q, 2q - 1, "mred": d met by MRedLazy of the
    difference, "halve": the parities of the words that reach halve}"""
    k = F.K(q)
    out = {"sum": set(), "dif": set(), "dif_arg": set(), "mred": set(), "halve": set()}
    xs, ys = np.asarray(x).reshape(-1, np.asarray(x).shape[-1]).tolist(), np.asarray(y).reshape(-1, np.asarray(y).shape[-1]).tolist()
    for rx, ry in zip(xs, ys):
        for u, (a, b) in enumerate(zip(rx, ry)):
            if form in POSITIONAL:
                b = F.MRed(b, tw[u], k)  # e +- MRed(o, w); a +- MRed(b, x)
            _near(out["sum"], a + b, q)
            _near(out["dif"], a + q - b, q)
            if a + q - b in (1, q, 2 * q - 1):
                out["dif_arg"].add((a + q - b - 1) // (q - 1))  # 0, 1, 2
            if form in ("split", "expand") and tw is not None:
                lazy = F.MRedLazy(a + q - b, tw[u], k)
                _near(out["mred"], lazy, q)
                if form == "split":
                    out["halve"].add(("even", F.CRed(a + b, q) & 1))
                    out["halve"].add(("odd", F.CRed(lazy, q) & 1))
    return out
