"""The reference's CKKS bridge restated on numpy and the oracle's ring primitives (a helper, not a test):
ring.FoldStandardToConjugateInvariant / UnfoldConjugateInvariantToStandard (ring/conjugate_invariant.go:3-44),
ckks.DomainSwitcher.ComplexToReal / RealToComplex (schemes/ckks/bridge.go:57-144) and
rlwe.KeyGenerator.GenEvaluationKeysForRingSwapNew (core/rlwe/keygenerator.go:211-233)."""
import numpy as np

from oracle import oracle as O
from tests.helpers import prod
from tests.rlwe_fixtures import SecretKey, gen_evaluation_key, phase, small_to_rns


def fold_index(N):
    """the table bridge.go:41 builds: AutomorphismNTTIndex(N, NthRoot = 2N, NthRoot - 1) of the standard ring of degree N"""
    return O.AutomorphismNTTIndex(N, 2 * N, 2 * N - 1)


def fold(a, q):
    """FoldStandardToConjugateInvariant on [limbs, N] -> [limbs, N/2]: AutomorphismNTTWithIndex over the first N/2 words
    (out[j] = in[index[j]]), then SubRing.Add with the input's first half (CRed(x + y), the sum wrapping in 64 bits)"""
    a = np.asarray(a, dtype=np.uint64)
    N = a.shape[-1]
    n = N // 2
    idx = fold_index(N)[:n].astype(np.int64)
    out = np.empty(a.shape[:-1] + (n,), dtype=np.uint64)
    for i in range(a.shape[0]):
        qi = np.uint64(int(q[i]))
        s = a[i][idx] + a[i][:n]  # uint64 arithmetic wraps, as Go's
        out[i] = np.where(s >= qi, s - qi, s)
    return out


def unfold(c):
    """UnfoldConjugateInvariantToStandard on [limbs, n] -> [limbs, 2n]: copy, then tmp2[jdx] = tmp1[idx] for idx = n-1 .. 0,
    jdx = n .. 2n-1"""
    c = np.asarray(c, dtype=np.uint64)
    return np.concatenate([c, c[..., ::-1]], axis=-1)


def _add(oQ, level, a, b):
    return O.Ring(oQ.N, oQ.moduli[: level + 1]).binop("Add", a[: level + 1], b[: level + 1])


def complex_to_real(oev, oQ, level, ct, ok):
    """bridge.go:87-91 on one ciphertext [2][limbs][N]: GadgetProduct(ct[1]) -> Add(ct[0]) -> Fold of both components"""
    gp = oev.GadgetProduct(level, ct[1][: level + 1], ok)
    q = oQ.moduli[: level + 1]
    return np.stack([fold(_add(oQ, level, gp[0], ct[0]), q), fold(gp[1], q)])


def real_to_complex(oev, oQ, level, ct, ok):
    """bridge.go:125-141 on one ciphertext [2][limbs][N/2]: Unfold of both components into opOut, GadgetProduct(opOut[1]),
    Add(opOut[0], .[0]) and CopyLvl(.[1])"""
    out = [unfold(ct[0][: level + 1]), unfold(ct[1][: level + 1])]
    gp = oev.GadgetProduct(level, out[1], ok)
    return np.stack([_add(oQ, level, out[0], gp[0]), gp[1][: level + 1].copy()])


def ci_mapped_to_standard(vals_ci):
    """the coefficients of skCIMappedToStandard: s(X + X^-1) written in Z[X]/(X^N+1), v[j] = s_j, v[N-j] = -s_j, v[n] = 0"""
    n = len(vals_ci)
    v = np.zeros(2 * n, dtype=np.int64)
    v[:n] = vals_ci
    v[n + 1:] = -np.asarray(vals_ci)[:0:-1]
    return v


def gen_ring_swap_keys(rng, oQ, oP, sk_std: SecretKey, vals_ci):
    """GenEvaluationKeysForRingSwapNew (keygenerator.go:211-233).  oQ, oP: the standard rings of degree N; vals_ci: the N/2
    ternary values of the conjugate-invariant secret.  Returns (skCI, skCIMappedToStandard, stdToci, ciToStd)."""
    n = oQ.N // 2
    ciQ, ciP = O.Ring(n, oQ.moduli, True), O.Ring(n, oP.moduli, True)
    sk_ci = SecretKey(rng, ciQ, ciP, vals=vals_ci)
    sk_map = SecretKey(rng, oQ, oP, vals=ci_mapped_to_standard(vals_ci))
    # :216 -- the reference gets the mapped key's Q part by unfolding the conjugate-invariant key's NTT words
    assert np.array_equal(sk_map.Q, unfold(sk_ci.Q)), "skCIMappedToStandard.Q != Unfold(skCI.Q)"
    std_to_ci = gen_evaluation_key(rng, oQ, oP, sk_std.Q, sk_map)  # GenEvaluationKey(skStd, skCIMappedToStandard)
    ci_to_std = gen_evaluation_key(rng, oQ, oP, sk_map.Q, sk_std)  # GenEvaluationKey(skCIMappedToStandard, skStd)
    return sk_ci, sk_map, std_to_ci, ci_to_std


# ---- the scheme side: encryption, decryption and the noise the bridge adds (tests/test_bridge_host.py derives the bounds) --------
SIGMA, EBOUND = 3.2, 19  # the fixtures' error: a rounded Gaussian of sigma 3.2 clipped at 19


def key_switch_noise_bound(N, q, p):
    """worst case, coefficient-wise, of one key switch at degree N with the fixtures' keys: the gadget product's
    digits N dmax EBOUND / P + 1, and ModDown's 1 per coefficient on both components against a ternary secret: 1 + N"""
    digits = O.BaseRNSDecompositionVectorSize(len(q) - 1, len(p) - 1)
    dmax = max(prod(q[d * len(p):(d + 1) * len(p)]) for d in range(digits))
    return (digits * N * dmax * EBOUND) // prod(p) + 1 + (1 + N)


def centred_phase(ring, ct, skQ):
    """the phase of ct under skQ, coefficient domain, centred modulo Q"""
    Q = prod(ring.moduli)
    ph = ring.INTT(phase(ring, ct, skQ))
    w = [(Q // int(qi)) * pow(Q // int(qi), -1, int(qi)) for qi in ring.moduli]
    out = []
    for j in range(ring.N):
        x = sum(int(ph[i, j]) * w[i] for i in range(len(w))) % Q
        out.append(x - Q if x > Q // 2 else x)
    return np.array(out, dtype=object)


def encrypt(rng, ring, skQ, m):
    """(m + e - a s, a) in the NTT domain of `ring` (either type); m: signed coefficients"""
    e = np.clip(np.rint(rng.normal(0.0, SIGMA, size=ring.N)), -EBOUND, EBOUND).astype(np.int64)
    a = np.stack([rng.integers(0, int(x), size=ring.N, dtype=np.uint64) for x in ring.moduli])
    pt = ring.NTT(small_to_rns(np.asarray(m, dtype=np.int64) + e, ring.moduli))
    return np.stack([ring.binop("Sub", pt, ring.binop("MulCoeffsMontgomery", a, skQ)), a])


def fold_ints(v):
    n = len(v) // 2
    return np.array([2 * v[0]] + [v[j] - v[2 * n - j] for j in range(1, n)], dtype=object)


def unfold_ints(v):
    n = len(v)
    return np.array(list(v) + [0] + [-v[j] for j in range(n - 1, 0, -1)], dtype=object)


def monomial_i(oQ):
    """NTT(X^(N/2)) in Montgomery form, read off the ring's roots: RootsForward[1] = MForm(psi^(N/2)) on the first half of the
    bit-reversed evaluation points and its negation on the second (X^(N/2) is a square root of -1: `i` on every slot)"""
    N = oQ.N
    mono = np.empty((len(oQ.moduli), N), dtype=np.uint64)
    for i, qi in enumerate(oQ.moduli):
        w = int(oQ.roots_forward(i)[1])
        mono[i, : N // 2], mono[i, N // 2:] = w, int(qi) - w
    x = np.zeros(N, dtype=np.int64)
    x[N // 2] = 1
    assert np.array_equal(mono, oQ.unop("MForm", oQ.NTT(small_to_rns(x, oQ.moduli))))
    return mono
