"""The ring-degree maps and the ring-packing kernels, stated twice (host only: no device, no numpy arithmetic on words).

1. The reference's own SEQUENCE OF CALLS, on the oracle: SwitchCiphertextRingDegreeNTT as INTT at N -> every gap-th coefficient ->
   NTT at n (core/rlwe/element.go:260-279), the replication (ring/operations.go:380), and the statements of Split, Merge, Expand
   and Pack of core/rlwe/ring_packing.go with MATERIALISED monomial tables (tests/ringpack_ref.py: a monomial, one NTT, repeated
   squaring).  These are what tests/test_gpu_ringmap_edges.py compares the device with.
2. The CLOSED FORM that include/hering_ringswitch.h and include/hering_ringpack.h promise, in Python integers, with the twiddle
   words read from the oracle's tables (roots_forward / roots_backward, Montgomery form).

tests/test_ringmap_host.py holds 1 against 2 on every ring, shape and family of tests/ringmap_edges.py."""
from __future__ import annotations

import functools

import numpy as np

from oracle import oracle as O
from tests import ringpack_ref as REF

U = np.uint64
R = 1 << 64


def arr(rows):
    return np.array(rows, dtype=U)


# ---------------------------------------------------------------------------------------------------------------
# 1. the reference's sequences of calls, on the oracle
# ---------------------------------------------------------------------------------------------------------------
def ref_down_ntt(a, q, N, gap, ci):
    """SwitchCiphertextRingDegreeNTT, N -> N / gap, on [limbs, N] (element.go:260-279)"""
    big, small = O.Ring(N, q[: a.shape[0]], ci), O.Ring(N // gap, q[: a.shape[0]], ci)
    return small.NTT(big.INTT(a)[:, ::gap].copy())


def ref_up_ntt(a, gap):
    """ring.MapSmallDimensionToLargerDimensionNTT (ring/operations.go:380)"""
    return np.repeat(a, gap, axis=1)


def ref_stride_down(a, gap):
    """SwitchCiphertextRingDegree, N -> N / gap (element.go:293-313)"""
    return a[..., ::gap].copy()


def ref_stride_up(a, gap, pre):
    """... n -> n gap: only the multiples of gap are written"""
    out = pre.copy()
    out[..., ::gap] = a
    return out


@functools.lru_cache(None)
def tables(N, mods, div):
    """GenXPow2NTT of the whole family (ring_packing.go:772-810) at the ring (N, mods), materialised on the oracle: [logN][limbs][N]"""
    return REF.GenXPow2NTT(O.Ring(N, list(mods)), N.bit_length() - 1, div)


def _tab(N, mods, div, k, limbs):
    return tables(N, tuple(mods), div)[k][:limbs]


def seq_split(t, mods, odd=True):
    """the ring maps of Split (:205-225) on one polynomial [limbs][N]: (even, odd or None)"""
    L, N = t.shape
    o = O.Ring(N, list(mods[:L]))
    even = REF.switch_down_ntt(t, o, N // 2)
    if not odd:
        return even, None
    return even, REF.switch_down_ntt(o.binop("MulCoeffsMontgomery", t, _tab(N, mods, True, 0, L)), o, N // 2)


def seq_merge(e, od, mods):
    """the ring maps of Merge (:410-417): [limbs][n] (+ [limbs][n] or None) -> [limbs][2n]"""
    L, n = e.shape
    out = REF.switch_up_ntt(e, 2)
    if od is None:
        return out
    return O.Ring(2 * n, list(mods[:L])).binop("MulCoeffsMontgomeryThenAdd", REF.switch_up_ntt(od, 2), _tab(2 * n, mods, False, 0, L), out)


def seq_expand(a, t, mods, k):
    """Expand's inner step (:541-550): (Add(c0, tmp), MulCoeffsMontgomery(Sub(c1, tmp), XInvPow2NTT[k]))"""
    L, N = a.shape
    o = O.Ring(N, list(mods[:L]))
    return o.binop("Add", a, t), o.binop("MulCoeffsMontgomery", o.binop("Sub", a, t), _tab(N, mods, True, k, L))


def seq_pack_pre(a, b, mods, k):
    """Pack's inner step before the automorphism (:697-721) on one polynomial of a pair: (a', b', T); an absent operand is None"""
    present = a if a is not None else b
    L, N = present.shape
    o = O.Ring(N, list(mods[:L]))
    if b is None:
        return a, None, a
    bx = o.binop("MulCoeffsMontgomery", b, _tab(N, mods, False, k, L))  # :703-704
    if a is None:
        return None, bx, bx  # :718
    return o.binop("Add", a, bx), b, o.binop("Sub", a, bx)  # :709-714 (b is discarded by the reference: left as it was)


def seq_pack_post(a, b, T, mods):
    """... and after it (:745-746, :763-764): (a', b')"""
    L, N = T.shape
    o = O.Ring(N, list(mods[:L]))
    if a is not None:
        return o.binop("Add", a, T), b
    return None, o.binop("Sub", b, T)


def seq_xpow2(N, mods, k, div, limbs):
    return _tab(N, mods, div, k, limbs)


# ---------------------------------------------------------------------------------------------------------------
# 2. the closed forms of the headers, in Python integers
# ---------------------------------------------------------------------------------------------------------------
def plain(w, q):
    """a twiddle word out of Montgomery form"""
    return w * pow(R, -1, q) % q


@functools.lru_cache(None)
def roots(N, mods, backward):
    """[limbs][N] RootsForward / RootsBackward of the standard ring, Montgomery form, as Python integers"""
    o = O.Ring(N, list(mods))
    return [(o.roots_backward(i) if backward else o.roots_forward(i)).tolist() for i in range(len(mods))]


def fold(a, mods, gap):
    """out[j] = gap^-1 sum_{s<gap} in[j gap + s] mod q"""
    out = []
    for row, q in zip(a.tolist(), mods):
        gi = pow(gap, -1, q)
        out.append([sum(row[j:j + gap]) * gi % q for j in range(0, len(row), gap)])
    return arr(out)


def xpow2(N, mods, k, div, limbs=None):
    """word j of XPow2NTT[k] / XInvPow2NTT[k]: w = Roots[(N >> (k+1)) + (j >> (k+1))] where bit k of j is clear, q - w where it is set"""
    return _xpow2(N, tuple(mods), k, bool(div))[:limbs]


@functools.lru_cache(None)
def _xpow2(N, mods, k, div):
    tw = roots(N, mods, div)
    out = []
    for i, q in enumerate(mods):
        w = [tw[i][(N >> (k + 1)) + (j >> (k + 1))] for j in range(N)]
        out.append([q - w[j] if (j >> k) & 1 else w[j] for j in range(N)])
    return out


def split(t, mods, odd=True):
    """even[j] = (a + b) / 2, odd[j] = (a - b) w^-1 / 2 with a = t[2j], b = t[2j+1], w^-1 = RootsBackward[N/2 + j]"""
    L, N = t.shape
    tw = roots(N, tuple(mods), True)
    ev, od = [], []
    for i, (row, q) in enumerate(zip(t.tolist(), mods)):
        h = pow(2, -1, q)
        ev.append([(row[2 * j] + row[2 * j + 1]) * h % q for j in range(N // 2)])
        od.append([(row[2 * j] - row[2 * j + 1]) * plain(tw[i][N // 2 + j], q) * h % q for j in range(N // 2)])
    return arr(ev), (arr(od) if odd else None)


def merge(e, od, mods):
    """out[2j], out[2j+1] = e[j] +- w o[j], w = RootsForward[N/2 + j]; without o the replication"""
    L, n = e.shape
    tw = roots(2 * n, tuple(mods), False)
    out = []
    for i, (row, q) in enumerate(zip(e.tolist(), mods)):
        o = od[i].tolist() if od is not None else [0] * n
        r = []
        for j in range(n):
            t = plain(tw[i][n + j], q) * o[j]
            r += [(row[j] + t) % q, (row[j] - t) % q]
        out.append(r)
    return arr(out)


def expand(a, t, mods, k):
    """(in + tmp, (in - tmp) X^(-2^k))"""
    L, N = a.shape
    x = xpow2(N, mods, k, True, L)
    s, d = [], []
    for i, (ra, rt, q) in enumerate(zip(a.tolist(), t.tolist(), mods)):
        s.append([(u + v) % q for u, v in zip(ra, rt)])
        d.append([(u - v) * plain(x[i][j], q) % q for j, (u, v) in enumerate(zip(ra, rt))])
    return arr(s), arr(d)


def pack_pre(a, b, mods, k):
    """a and b: T = a - b x, a <- a + b x;  a only: T = a;  b only: b <- b x, T = b x  (x = X^(2^k)): (a', b', T)"""
    if b is None:
        return a, None, a
    L, N = b.shape
    x = xpow2(N, mods, k, False, L)
    bx = [[v * plain(x[i][j], q) % q for j, v in enumerate(row)] for i, (row, q) in enumerate(zip(b.tolist(), mods))]
    if a is None:
        return None, arr(bx), arr(bx)
    al = a.tolist()
    return (arr([[(u + v) % q for u, v in zip(al[i], bx[i])] for i, q in enumerate(mods[:L])]), b,
            arr([[(u - v) % q for u, v in zip(al[i], bx[i])] for i, q in enumerate(mods[:L])]))


def pack_post(a, b, T, mods):
    """a present: a <- a + T;  b only: b <- b - T: (a', b')"""
    tl = T.tolist()
    if a is not None:
        return arr([[(u + v) % q for u, v in zip(row, tl[i])] for i, (row, q) in enumerate(zip(a.tolist(), mods))]), b
    return None, arr([[(u - v) % q for u, v in zip(row, tl[i])] for i, (row, q) in enumerate(zip(b.tolist(), mods))])
