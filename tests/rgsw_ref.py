"""rgsw.Evaluator.ExternalProduct (core/rgsw/evaluator.go:39-280) restated on the oracle's ring primitives, branch by branch,
in the reference's loop order and with its reduce schedule -- NOT as a composition of GadgetProductLazy (tests/test_rgsw_host.py
holds the two against each other).

An RGSW ciphertext is a pair of oracle EvaluationKeys (elements.go:12, `Value [2]rlwe.GadgetCiphertext`): rgsw[k].q[d, c, u] is
el.Value[i][j][c].Q.Coeffs[u] of component k, digit d = (RNS digit i, window j) flattened as the key stores them.
Polynomials are [limbs, N] uint64, NTT domain; ct = [2, levelQ + 1, N]."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

U64 = np.uint64


_SUBRINGS: dict = {}


def _at(ring: O.Ring, lo: int, hi: int) -> O.Ring:
    """limbs lo..hi-1 of a ring, of the ring's own type"""
    key = (ring.N, tuple(ring.moduli[lo:hi]), ring.conjugate_invariant)
    if key not in _SUBRINGS:
        _SUBRINGS[key] = O.Ring(ring.N, ring.moduli[lo:hi], ring.conjugate_invariant)
    return _SUBRINGS[key]


def _sub(ring: O.Ring, u: int) -> O.Ring:
    """ring.SubRings[u] as a ring of its own (SubRing.NTTLazy, SubRing.MulCoeffsMontgomery...)"""
    return _at(ring, u, u + 1)


def _windows(evk: O.EvaluationKey, levelQ: int):
    """BaseTwoDecompositionVectorSize (gadgetciphertext.go): windows of each RNS digit; one with BaseTwoDecomposition == 0"""
    return [evk.nj[i] if evk.pw2 else 1 for i in range(levelQ + 1)]


def mask_vec(p1: np.ndarray, w: int, mask: int) -> np.ndarray:
    """ring.MaskVec (ring/vec_ops.go:870)"""
    return (p1 >> U64(w)) & U64(mask)


def external_product_32bit(ringQ: O.Ring, ct: np.ndarray, rgsw) -> np.ndarray:
    """externalProduct32Bit (:84-128) and the two IMForm of ExternalProduct (:61-63): plain 64-bit products summed with
    wrap-around, exactly as the reference's MulCoeffsLazy / MulCoeffsLazyThenAddLazy"""
    s = _sub(ringQ, 0)
    pw2 = rgsw[0].pw2
    mask = (1 << pw2) - 1
    acc0 = acc1 = None
    for i, el in enumerate(rgsw):
        buffQ = s.INTT(ct[i][:1])
        for j in range(el.q.shape[0]):
            cw = mask_vec(buffQ[0], j * pw2, mask)
            cwNTT = s.NTTLazy(cw[None, :])[0]
            with np.errstate(over="ignore"):
                if j == 0 and i == 0:
                    acc0 = el.q[j, 0, 0] * cwNTT
                    acc1 = el.q[j, 1, 0] * cwNTT
                else:
                    acc0 = acc0 + el.q[j, 0, 0] * cwNTT
                    acc1 = acc1 + el.q[j, 1, 0] * cwNTT
    return np.stack([s.unop("IMForm", acc0[None, :]), s.unop("IMForm", acc1[None, :])])


def external_product_bit_decomp(ringQ: O.Ring, ringP: O.Ring | None, ct: np.ndarray, rgsw):
    """externalProductInPlaceSinglePAndBitDecomp (:130-204) -> (cQ [2, levelQ + 1, N], cP [2, levelP + 1, N])"""
    levelQ, levelP = rgsw[0].LevelQ(), rgsw[0].LevelP()
    N = ringQ.N
    pw2 = rgsw[0].pw2
    mask = (1 << pw2) - 1
    if mask == 0:
        mask = 0xFFFFFFFFFFFFFFFF
    nj = _windows(rgsw[0], levelQ)
    cQ = np.zeros((2, levelQ + 1, N), dtype=U64)
    cP = np.zeros((2, levelP + 1, N), dtype=U64)
    subQ = _at(ringQ, 0, levelQ + 1)
    for k, el in enumerate(rgsw):
        buffQ = subQ.INTT(ct[k][: levelQ + 1])
        d = 0
        for i in range(levelQ + 1):
            for j in range(nj[i]):
                cw = mask_vec(buffQ[i], j * pw2, mask)
                first = k == 0 and i == 0 and j == 0
                for u in range(levelQ + 1):
                    s = _sub(ringQ, u)
                    cwNTT = s.NTTLazy(cw[None, :])
                    for c in range(2):
                        key = el.q[d, c, u][None, :]
                        cQ[c, u] = (s.binop("MulCoeffsMontgomery", key, cwNTT) if first
                                    else s.binop("MulCoeffsMontgomeryThenAdd", key, cwNTT, cQ[c, u][None, :]))[0]
                if ringP is not None:
                    for u in range(levelP + 1):
                        s = _sub(ringP, u)
                        cwNTT = s.NTTLazy(cw[None, :])
                        for c in range(2):
                            key = el.p[d, c, u][None, :]
                            cP[c, u] = (s.binop("MulCoeffsMontgomery", key, cwNTT) if first
                                        else s.binop("MulCoeffsMontgomeryThenAdd", key, cwNTT, cP[c, u][None, :]))[0]
                d += 1
    return cQ, cP


def external_product_multiple_p(oev: O.Evaluator, ct: np.ndarray, rgsw):
    """externalProductInPlaceMultipleP (:206-280) with its reduce schedule (QiOverflowMargin >> 1, PiOverflowMargin >> 1)"""
    ringQ, ringP = oev.ringQ, oev.ringP
    levelQ, levelP = rgsw[0].LevelQ(), rgsw[0].LevelP()
    N = ringQ.N
    subQ, subP = _at(ringQ, 0, levelQ + 1), _at(ringP, 0, levelP + 1)
    beta = O.BaseRNSDecompositionVectorSize(levelQ, levelP)
    QiOverF = int(2.0 ** 64 / float(max(ringQ.moduli[: levelQ + 1]))) >> 1
    PiOverF = int(2.0 ** 64 / float(max(ringP.moduli[: levelP + 1]))) >> 1
    cQ = np.zeros((2, levelQ + 1, N), dtype=U64)
    cP = np.zeros((2, levelP + 1, N), dtype=U64)
    reduce = 0
    for k, el in enumerate(rgsw):
        # DecomposeSingleNTT(levelQ, levelP, levelP + 1, i, c2NTT, c2InvNTT, ...) for every i is DecomposeNTT (evaluator.go)
        dq, dp = oev.DecomposeNTT(levelQ, levelP, levelP + 1, ct[k][: levelQ + 1])
        for i in range(beta):
            for c in range(2):
                if k == 0 and i == 0:
                    cQ[c] = subQ.binop("MulCoeffsMontgomeryLazy", el.q[i, c, : levelQ + 1], dq[i])
                    cP[c] = subP.binop("MulCoeffsMontgomeryLazy", el.p[i, c, : levelP + 1], dp[i])
                else:
                    cQ[c] = subQ.binop("MulCoeffsMontgomeryLazyThenAddLazy", el.q[i, c, : levelQ + 1], dq[i], cQ[c])
                    cP[c] = subP.binop("MulCoeffsMontgomeryLazyThenAddLazy", el.p[i, c, : levelP + 1], dp[i], cP[c])
            if reduce % QiOverF == QiOverF - 1:
                cQ = np.stack([subQ.unop("Reduce", cQ[0]), subQ.unop("Reduce", cQ[1])])
            if reduce % PiOverF == PiOverF - 1:
                cP = np.stack([subP.unop("Reduce", cP[0]), subP.unop("Reduce", cP[1])])
            reduce += 1
    if reduce % QiOverF != 0:
        cQ = np.stack([subQ.unop("Reduce", cQ[0]), subQ.unop("Reduce", cQ[1])])
    if reduce % PiOverF != 0:
        cP = np.stack([subP.unop("Reduce", cP[0]), subP.unop("Reduce", cP[1])])
    return cQ, cP


def takes_32bit_branch(ringQ: O.Ring, rgsw) -> bool:
    """the condition of :60"""
    return rgsw[0].LevelQ() == 0 and rgsw[0].LevelP() == -1 and (int(ringQ.moduli[0]) >> 29) == 0


def wrap_bound_holds(ringQ: O.Ring, rgsw, key_mul: int = 1) -> bool:
    """2 D W (M q - 1) < 2^64 with W = 6q - 2 the largest word of NTTLazy (ring/ntt.go:133) and key words below M q (M = 1:
    canonical keys): the 32-bit branch's sum cannot wrap"""
    q = int(ringQ.moduli[0])
    return 2 * rgsw[0].q.shape[0] * (6 * q - 2) * (key_mul * q - 1) < (1 << 64)


def key_words_in_domain(ringQ: O.Ring, ringP: O.Ring | None, rgsw, key_mul: int) -> bool:
    """Whether the reference's arithmetic is exact with key words below M q (include/hering_rgsw.h, "Key words"): every
    product MRed / MRedLazy(key, y) has key * y < q 2^64 -- y an NTTLazy word, at most 6q - 2, in the bit-window branch and a word
    below 2q in branch M -- and the 32-bit branch's plain sum stays below 2^64."""
    levelQ, levelP = rgsw[0].LevelQ(), rgsw[0].LevelP()
    if levelP < 1 and takes_32bit_branch(ringQ, rgsw):
        return wrap_bound_holds(ringQ, rgsw, key_mul)
    mods = [int(q) for q in ringQ.moduli[: levelQ + 1]] + ([int(p) for p in ringP.moduli[: levelP + 1]] if levelP >= 0 else [])
    ymax = (lambda q: 2 * q - 1) if levelP >= 1 else (lambda q: 6 * q - 2)
    return all(key_mul * q < (1 << 64) and (key_mul * q - 1) * ymax(q) < (q << 64) for q in mods)


def external_product(oev: O.Evaluator, ct: np.ndarray, rgsw, force_bit_decomp: bool = False, with_p_coeffs: bool = False):
    """ExternalProduct (:39-82) -> [2, levelQ + 1, N]; force_bit_decomp: take :66 where :60 would choose the 32-bit branch.
    with_p_coeffs: -> (product, [2, levelP + 1, N]) with the coefficients of the P accumulator, the residues ModDown lifts
    (INTT of the accumulator's P part, ring/basis_extension.go:247); levelP >= 0 only."""
    ringQ, ringP = oev.ringQ, oev.ringP
    levelQ, levelP = rgsw[0].LevelQ(), rgsw[0].LevelP()
    assert levelP >= 0 or not with_p_coeffs
    if levelP < 1:
        if takes_32bit_branch(ringQ, rgsw) and not force_bit_decomp:
            return external_product_32bit(ringQ, ct, rgsw)
        cQ, cP = external_product_bit_decomp(ringQ, ringP, ct, rgsw)
        if levelP < 0:
            return cQ.copy()
    else:
        cQ, cP = external_product_multiple_p(oev, ct, rgsw)
    be = O.BasisExtender(ringQ, ringP)
    out = np.stack([be.ModDownQPtoQNTT(levelQ, levelP, cQ[c], cP[c]) for c in range(2)])
    if with_p_coeffs:
        subP = _at(ringP, 0, levelP + 1)
        return out, np.stack([subP.INTT(cP[c]) for c in range(2)])
    return out


def window_counts(moduli, pw2: int):
    """BaseTwoDecompositionVectorSize of the reference's NewCiphertext: ceil(bits(q_i) / pw2) windows of limb i"""
    return [(int(q).bit_length() + pw2 - 1) // pw2 for q in moduli]


def row_words(kind_of, rng, moduli, N, D):
    """[D, 2, limbs, N] key words: kind_of(rng, moduli, N) -> [limbs, N] is called once per (digit, component) row"""
    return np.stack([np.stack([kind_of(rng, moduli, N) for _c in range(2)]) for _d in range(D)])


def uniform_rgsw(rng, ringQ: O.Ring, ringP: O.Ring | None, pw2: int, rns_p: bool = False, levelQ: int | None = None, nj=None,
                 words=None):
    """Two uniformly random gadget ciphertexts of the shape the reference's NewCiphertext gives: pw2 > 0 -- bit windows, one
    digit per Q limb; pw2 == 0 -- RNS digits (one uncentred window per limb where there is a single special prime).
    levelQ: keys of limbs 0..levelQ of ringQ (NewCiphertext(params, levelQ, levelP, ...) below the ring's top level).
    nj: window counts other than the reference's (a key may carry more windows than its limb has bits: the upper ones are
    windows of zero).  words(rng, moduli, N) -> [limbs, N]: another source of key words than the uniform one."""
    N = ringQ.N
    qmods = list(ringQ.moduli) if levelQ is None else list(ringQ.moduli[: levelQ + 1])
    LQ, LP = len(qmods), (len(ringP.moduli) if ringP is not None else 0)
    if pw2:
        nj = list(nj) if nj is not None else window_counts(qmods, pw2)
        assert len(nj) == LQ
        D = sum(nj)
    else:
        nj = None
        D = O.BaseRNSDecompositionVectorSize(LQ - 1, LP - 1)
    out = []
    if words is not None:
        for _ in range(2):
            kq = row_words(words, rng, qmods, N, D)
            kp = row_words(words, rng, list(ringP.moduli), N, D) if LP else np.zeros((D, 2, 0, N), dtype=U64)
            out.append(O.EvaluationKey(kq, kp, pw2=pw2, nj=nj))
        return out
    for _ in range(2):
        kq = np.stack([np.stack([np.stack([rng.integers(0, int(q), size=N, dtype=U64) for q in qmods]) for _c in range(2)]) for _d in range(D)])
        if LP:
            kp = np.stack([np.stack([np.stack([rng.integers(0, int(q), size=N, dtype=U64) for q in ringP.moduli]) for _c in range(2)]) for _d in range(D)])
        else:
            kp = np.zeros((D, 2, 0, N), dtype=U64)
        out.append(O.EvaluationKey(kq, kp, pw2=pw2, nj=nj))
    return out


LIFT_TARGETS = ("(p-1)/2", "(p+1)/2", "0", "p-1")


def lift_targets(p: int, N: int) -> np.ndarray:
    """N residues mod p cycling through (p - 1) / 2, (p + 1) / 2, 0 and p - 1: the two sides of ModDown's centred lift
    (v > (p - 1) / 2 ? v - p : v) and the ends of the range"""
    p = int(p)
    return np.array([((p - 1) // 2, (p + 1) // 2, 0, p - 1)[i % 4] for i in range(N)], dtype=U64)


def planted_rgsw(rng, ringQ: O.Ring, ringP: O.Ring, pw2: int, component: int, levelQ: int | None = None):
    """An RGSW pair whose product with (NTT(1), 0) has lift_targets(p, N) as the coefficients of output component `component`'s P
    accumulator (and zero as the other's): every P row is zero except digit 0 of rgsw[0], component `component`, which holds
    MForm(NTT_p(targets)); the Q rows are uniform.  Window 0 of limb 0 of INTT(NTT(1)) = 1 is the constant 1, whose transform is
    all ones, so that row enters the accumulator as it stands; every other window is zero or meets a zero P row."""
    assert ringP is not None and len(ringP.moduli) == 1
    out = uniform_rgsw(rng, ringQ, ringP, pw2, levelQ=levelQ)
    for k in out:
        k.p[...] = 0
    t = lift_targets(ringP.moduli[0], ringQ.N)[None, :]
    out[0].p[0, component] = ringP.unop("MForm", ringP.NTT(t))
    return [O.EvaluationKey(k.q, k.p, pw2=pw2, nj=k.nj if pw2 else None) for k in out]


def ntt_of_one(ringQ: O.Ring, nlimbs: int) -> np.ndarray:
    """NTT(1): the constant polynomial 1 is all ones in every limb"""
    return np.ones((nlimbs, ringQ.N), dtype=U64)


def all_mask_coeffs(q: int, pw2: int, N: int) -> np.ndarray:
    """The largest coefficient below q whose windows of pw2 bits are all equal to the mask, except the top one, which is what q
    leaves of it (t - 1 with t = q >> (nj - 1) pw2 the top window of q itself)"""
    q = int(q)
    s = ((q.bit_length() + pw2 - 1) // pw2 - 1) * pw2
    return np.full(N, ((q >> s) << s) - 1, dtype=U64)


# ---- the helpers of :283-356 on pairs of oracle keys; every function returns new keys ------------------------------------------------
def _map_rows(ringQ, ringP, rgsw_in, rgsw_out, fq, fp):
    """opOut.Value[k].Value[i][j][c] = f(ctIn..., opOut...) over every (k, digit, component), Q and P parts"""
    out = []
    subQ = _at(ringQ, 0, rgsw_in[0].LevelQ() + 1)
    subP = _at(ringP, 0, rgsw_in[0].LevelP() + 1) if rgsw_in[0].LevelP() >= 0 else None
    for k in range(2):
        kq, kp = rgsw_out[k].q.copy(), rgsw_out[k].p.copy()
        for d in range(kq.shape[0]):
            for c in range(2):
                kq[d, c] = fq(subQ, rgsw_in[k].q[d, c], kq[d, c])
                if subP is not None:
                    kp[d, c] = fp(subP, rgsw_in[k].p[d, c], kp[d, c])
        out.append(O.EvaluationKey(kq, kp, pw2=rgsw_out[k].pw2, nj=rgsw_out[k].nj if rgsw_out[k].pw2 else None))
    return out


def add_lazy_ciphertext(ringQ, ringP, el, opOut):
    """AddLazy, *Ciphertext case (:308-316)"""
    f = lambda r, a, o: r.binop("AddLazy", o, a)
    return _map_rows(ringQ, ringP, el, opOut, f, f)


def add_lazy_plaintext(ringQ, ringP, pt, opOut):
    """AddLazy, *Plaintext case (:285-307); pt [windows, limbs, N]"""
    nQ = opOut[0].LevelQ() + 1
    nP = max(opOut[0].LevelP() + 1, 1)
    nj = _windows(opOut[0], nQ - 1) if opOut[0].pw2 else [1] * opOut[0].q.shape[0]
    kq = [opOut[0].q.copy(), opOut[1].q.copy()]
    with np.errstate(over="ignore"):
        d = 0
        for i in range(len(nj)):
            start, end = i * nP, min((i + 1) * nP, nQ)
            for j in range(nj[i]):
                for k in range(start, end):
                    kq[0][d, 0, k] = kq[0][d, 0, k] + pt[j, k]
                    kq[1][d, 1, k] = kq[1][d, 1, k] + pt[j, k]
                d += 1
    return [O.EvaluationKey(kq[k], opOut[k].p, pw2=opOut[k].pw2, nj=opOut[k].nj if opOut[k].pw2 else None) for k in range(2)]


def reduce(ringQ, ringP, ctIn, opOut):
    """Reduce (:323)"""
    f = lambda r, a, o: r.unop("Reduce", a)
    return _map_rows(ringQ, ringP, ctIn, opOut, f, f)


def mul_by_xpow_alpha_minus_one_lazy(ringQ, ringP, ctIn, xQ, xP, opOut, then_add=False):
    """MulByXPowAlphaMinusOneLazy (:335) / ...ThenAddLazy (:347)"""
    name = "MulCoeffsMontgomeryLazyThenAddLazy" if then_add else "MulCoeffsMontgomeryLazy"
    fq = lambda r, a, o: r.binop(name, a, xQ, o if then_add else None)
    fp = lambda r, a, o: r.binop(name, a, xP, o if then_add else None)
    return _map_rows(ringQ, ringP, ctIn, opOut, fq, fp)


def xpow_alpha_minus_one(ring: O.Ring, alpha: int) -> np.ndarray:
    """X^alpha - 1 (alpha in (-N, N), X^-a = -X^(N-a)) in NTT + Montgomery form, as blindrot's evaluator precomputes it"""
    N = ring.N
    c = np.zeros(N, dtype=np.int64)
    a = alpha % (2 * N)
    c[a % N] += 1 if a < N else -1
    c[0] -= 1
    res = np.stack([np.where(c < 0, np.uint64(q) - (-c).astype(np.uint64), c.astype(np.uint64)) % np.uint64(q) for q in ring.moduli])
    return ring.unop("MForm", ring.NTT(res))
