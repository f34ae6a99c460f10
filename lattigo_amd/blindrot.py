"""Host-side mirror of core/rgsw/blindrot (blindrot.go, evaluator.go, keys.go, utils.go): blind rotation of LWE samples
extracted from an RLWE ciphertext, backed by include/hering_blindrot.h.  The accumulators of all requested slots are ONE batched
ciphertext and BlindRotateCore is one call for all of them; the prologue of Evaluate (the switch to modulus 2N) runs on the host
in exact integer arithmetic, as the reference's runs on big integers."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import rgsw, rlwe
from ._lib import H, check, load, u64p
from .ring import Poly, Ring

windowSize = 10  # keys.go:14
GaloisGen = rlwe.GaloisGen


def GaloisElements(N: int):
    """the Galois elements BlindRotateCore asks for (keys.go:94-99): GaloisGen^1 .. GaloisGen^windowSize and 2N - GaloisGen"""
    return [rlwe.GaloisElement(2 * N, i + 1) for i in range(windowSize)] + [2 * N - GaloisGen]


def _scaleUp(value: float, scale: float, Q: int) -> int:
    """utils.go:26: round(|scale * value|) mod Q in double precision, negated for a negative value (0 becomes Q there)"""
    x = -scale * value if value < 0 else scale * value
    res = int(math.floor(x + 0.5)) % Q
    return Q - res if value < 0 else res


def _normalizeInv(x: float, a: float, b: float) -> float:
    return (x * (b - a) + b + a) / 2.0


def InitTestPolynomial(g, scale: float, ringQ: Ring, a: float, b: float) -> Poly:
    """blindrot.go:12: the test polynomial of g on [a, b] at `scale`, NTT domain, one polynomial (batch 1) of ringQ's level"""
    N = ringQ.N
    moduli = [int(q) for q in ringQ.ModuliChain()[: ringQ.Level() + 1]]
    interval = 2.0 / float(N)
    sf64 = float(scale)
    F = np.zeros((len(moduli), N), dtype=np.uint64)
    for j, qi in enumerate(moduli):
        for i in range((N >> 1) + 1):
            F[j, i] = _scaleUp(g(_normalizeInv(-interval * float(i), a, b)), sf64, qi)
        for i in range((N >> 1) + 1, N):
            F[j, i] = _scaleUp(-g(_normalizeInv(interval * float(N - i), a, b)), sf64, qi)
    out = Poly(ringQ, len(moduli), 1).upload(F[None])
    ringQ.NTT(out, out)
    return out


class GaloisKeySet:
    """The automorphism keys of a blind rotation resident on the device with their index tables
    (BlindRotationEvaluationKeySet.GetEvaluationKeySet, keys.go:41), addressed by index from AutomorphismSelect."""

    def __init__(self, evaluator: rlwe.Evaluator, keys: dict):
        self.galEls = [int(g) for g in keys]
        self.keys = [keys[g] for g in keys]
        n = len(self.keys)
        g = (C.c_uint64 * n)(*self.galEls)
        k = (H * n)(*[x.h for x in self.keys])
        h = H()
        check(load().he_galois_keyset_create(evaluator.h, n, g, k, C.byref(h)))
        self.h = h.value

    def __len__(self):
        return len(self.keys)

    def index(self, galEl: int) -> int:
        return self.galEls.index(int(galEl))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                load().he_galois_keyset_destroy(self.h)
                self.h = None
        except Exception:
            pass


def AutomorphismSelect(evaluator: rlwe.Evaluator, ctIn, keys: GaloisKeySet, sel, opOut):
    """Batch entry b of ctIn through rlwe.Evaluator.Automorphism with keys[sel[b]]; sel[b] == -1 passes the entry through.  One
    launch, small rings and base-2 gadget keys only (hering_blindrot.h)."""
    s = np.ascontiguousarray(sel, dtype=np.int32)
    check(load().he_automorphism_ct_select(evaluator.h, ctIn[0].h, ctIn[1].h, keys.h, s.ctypes.data_as(C.POINTER(C.c_int32)),
                                           int(s.size), opOut[0].h, opOut[1].h))


class MemBlindRotationEvaluationKeySet:
    """keys.go:32: BlindRotationKeys [n_lwe] rgsw.Ciphertext (RGSW(X^s[i])) and AutomorphismKeys {Galois element: EvaluationKey},
    both made resident as tables the select forms index"""

    def __init__(self, evaluator: rgsw.Evaluator, BlindRotationKeys, AutomorphismKeys: dict):
        self.BlindRotationKeys = list(BlindRotationKeys)
        self.AutomorphismKeys = dict(AutomorphismKeys)
        self.rgsw = rgsw.KeySet(evaluator, self.BlindRotationKeys)
        self.galois = GaloisKeySet(evaluator, self.AutomorphismKeys)

    def GetBlindRotationKey(self, i: int) -> rgsw.Ciphertext:
        return self.BlindRotationKeys[i]

    def GetEvaluationKeySet(self) -> GaloisKeySet:
        return self.galois


def GenEvaluationKeyNew(paramsRLWE: rgsw.Evaluator, skRLWE, paramsLWE: Ring, skLWE, evkParams=None, prng=None, prngKeyGen=None,
                        XeSigma: float | None = None, XeBound: float | None = None) -> MemBlindRotationEvaluationKeySet:
    """keys.go:46-108 on the device (he_blindrot_gen_evaluation_key): RGSW(X^s[i]) for every coefficient of skLWE (an rlwe SecretKey
    of the ring paramsLWE; limb 0 of its Q part is read) and the Galois keys of GaloisElements(N), under skRLWE, at the levels and
    BaseTwoDecomposition of evkParams (keygen.EvaluationKeyParameters).  prng: the source of the RGSW ciphertexts; prngKeyGen: that
    of the Galois keys (None: prng, the RGSW ciphertexts drawing first).  An exact function of the byte streams."""
    from . import keygen as _kg
    from .sampling import PRNG
    prng = PRNG() if prng is None else prng
    dist = (_kg.DefaultXeSigma if XeSigma is None else XeSigma, _kg.DefaultXeBound if XeBound is None else XeBound)
    kgen = _kg.KeyGenerator(paramsRLWE, prng if prngKeyGen is None else prngKeyGen, _kg.DefaultXsP, *dist)
    levelQ, levelP, pw2 = kgen._resolve(evkParams)
    enc = rgsw.Encryptor(paramsRLWE, prng, skRLWE, *dist)
    n = paramsLWE.N
    cts = [rgsw.NewCiphertext(paramsRLWE, levelQ, levelP, pw2) for _ in range(n)]
    galEls = GaloisElements(paramsRLWE.ringQ.N)
    params = _kg.EvaluationKeyParameters(levelQ, levelP, pw2)
    gks = [kgen.NewEvaluationKey(params) for _ in galEls]
    a0 = (H * n)(*[c.Value[0].h for c in cts])
    a1 = (H * n)(*[c.Value[1].h for c in cts])
    ag = (H * len(gks))(*[k.h for k in gks])
    rc = load().he_blindrot_gen_evaluation_key(enc.h, kgen.h, paramsLWE.h, skLWE.Q.h, n, a0, a1, ag)
    (prngKeyGen if prngKeyGen is not None and prngKeyGen.error is not None else prng).check(rc)  # (the reader's exception, if it raised one)
    return MemBlindRotationEvaluationKeySet(paramsRLWE, cts, dict(zip(galEls, gks)))


def Schedule(logN: int, a):
    """The operations BlindRotateCore applies for the row a, in order: ("automorphism", Galois element) or
    ("external_product", key index).  Host only (he_debug_blindrot_schedule)."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    n = C.c_size_t()
    L = load()
    check(L.he_debug_blindrot_schedule(logN, a.ctypes.data_as(u64p), int(a.size), None, 0, C.byref(n)))
    ops = np.zeros(2 * max(n.value, 1), dtype=np.uint64)
    check(L.he_debug_blindrot_schedule(logN, a.ctypes.data_as(u64p), int(a.size), ops.ctypes.data_as(u64p), n.value, C.byref(n)))
    return [("external_product" if ops[2 * i] else "automorphism", int(ops[2 * i + 1])) for i in range(n.value)]


def Rounds(logN: int, rows):
    """The merged rounds of a batch of rows [batch][n_lwe]: a list of (gal [batch], prod [batch]) -- the Galois element of each
    entry's automorphism in that round (0: none) and the key of its external product (-1: none)."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    B, n_lwe = rows.shape
    n = C.c_size_t()
    L = load()
    check(L.he_debug_blindrot_rounds(logN, rows.ctypes.data_as(u64p), B, n_lwe, None, 0, C.byref(n)))
    out = np.zeros((max(n.value, 1), 2, B), dtype=np.int64)
    check(L.he_debug_blindrot_rounds(logN, rows.ctypes.data_as(u64p), B, n_lwe, out.ctypes.data_as(C.POINTER(C.c_int64)), n.value, C.byref(n)))
    return [(out[r, 0].copy(), out[r, 1].copy()) for r in range(n.value)]


def _crt(limbs, moduli):
    """PolyToBigint(pol, 1, .): the coefficients in [0, Q)"""
    Q = math.prod(moduli)
    w = [(Q // q) * pow(Q // q, -1, q) for q in moduli]
    return [sum(int(limbs[i][j]) * w[i] for i in range(len(moduli))) % Q for j in range(limbs.shape[1])], Q


def modSwitchRLWETo2N(coeffs, Q: int, twoN: int, makeOdd: bool):
    """evaluator.go:284: round(x 2N / Q) mod 2N (bignum.DivRound on non-negative integers: halves round up); makeOdd flips the
    lowest bit of even words other than 0"""
    out = []
    for x in coeffs:
        v = ((2 * x * twoN + Q) // (2 * Q)) & (twoN - 1)
        if makeOdd and v & 1 == 0 and v != 0:
            v ^= 1
        out.append(v)
    return out


def mulBySmallMonomialMod2N(mask: int, pol: list, n: int) -> list:
    """utils.go:11: pol * X^n with 0 <= n < N, coefficients mod 2N"""
    if n == 0:
        return pol
    N = len(pol)
    pol = pol[N - n:] + pol[:N - n]
    for j in range(n):
        pol[j] = -pol[j] & mask
    return pol


class Evaluator:
    """blindrot.Evaluator (evaluator.go:16).  paramsBR: the rgsw.Evaluator of the blind rotation's ring; paramsLWE: the Ring of
    the LWE samples; NTTFlag: paramsBR.NTTFlag(), the domain of the results."""

    def __init__(self, paramsBR: rgsw.Evaluator, paramsLWE: Ring, NTTFlag: bool = True):
        self.eval = paramsBR
        self.ringQBR = paramsBR.ringQ
        self.ringQLWE = paramsLWE
        self.NTTFlag = NTTFlag

    def BlindRotateCore(self, a, acc, BRK: MemBlindRotationEvaluationKeySet):
        """evaluator.go:135 for every batch entry of acc, in place: a is [batch][n_lwe] (or one row for a batch of one)"""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        if a.ndim == 1:
            a = a[None]
        check(load().he_blind_rotate_core(self.eval.h, a.ctypes.data_as(u64p), int(a.shape[0]), int(a.shape[1]), acc[0].h, acc[1].h,
                                          BRK.rgsw.h, BRK.galois.h))

    def Evaluate(self, ct, testPolyWithSlotIndex: dict, BRK: MemBlindRotationEvaluationKeySet, isNTT: bool = True, level=None):
        """evaluator.go:49: ct = [Poly, Poly] over the LWE ring (batch 1) at `level`; testPolyWithSlotIndex {slot: test polynomial
        (Poly, NTT domain)}.  Returns {slot: [Poly, Poly]} over the blind rotation's ring."""
        brk = BRK.GetBlindRotationKey(0)
        levelBR = brk.LevelQ()
        level = ct[0].Level() if level is None else level
        ringQBR = self.ringQBR.AtLevel(levelBR)
        ringQLWE = self.ringQLWE.AtLevel(level)
        NLWE, NBR = ringQLWE.N, ringQBR.N
        words = []
        for c in ct:
            if isNTT:
                t = Poly(self.ringQLWE, level + 1, 1, zero=False)
                ringQLWE.INTT(c, t)
                c = t
            words.append(c.download()[0, : level + 1])
        moduli = [int(q) for q in self.ringQLWE.ModuliChain()[: level + 1]]
        twoN = NBR << 1
        mask = twoN - 1
        c1, Q = _crt(words[1], moduli)
        c0, _ = _crt(words[0], moduli)
        tmp1 = modSwitchRLWETo2N(c1, Q, twoN, True)
        # Convolution(a, sk) -> DotProd(a, sk): a_0, -a_{N-1}, ..., -a_1 (:79-87)
        aRLWE = [tmp1[0]] + [-tmp1[NLWE - j] & mask for j in range(1, NLWE)]
        bRLWE = modSwitchRLWETo2N(c0, Q, twoN, False)
        slots = [i for i in range(NLWE) if i in testPolyWithSlotIndex]
        if not slots:
            return {}
        rows, prev = [], 0
        for index in slots:
            aRLWE = mulBySmallMonomialMod2N(mask, aRLWE, index - prev)
            prev = index
            rows.append(list(aRLWE))
        B, L = len(slots), levelBR + 1
        # Acc = (f(X^-g) X^(-g b), 0) (:108-113): NewMonomialXi(b), NTT, MForm, times the test polynomial, AutomorphismNTT by 2N - g
        qBR = [int(q) for q in self.ringQBR.ModuliChain()[:L]]
        Xb = np.zeros((B, L, NBR), dtype=np.uint64)
        for e, index in enumerate(slots):
            b = bRLWE[index] & mask
            for k, q in enumerate(qBR):
                if b >= NBR:
                    Xb[e, k, b - NBR] = q - 1
                else:
                    Xb[e, k, b] = 1
        xb = Poly(self.ringQBR, L, B).upload(Xb)
        ringQBR.NTT(xb, xb)
        ringQBR.MForm(xb, xb)
        test = Poly(self.ringQBR, L, B, zero=False)
        for e, index in enumerate(slots):
            test.CopyBatch(levelBR, e, testPolyWithSlotIndex[index], 0, 1)
        acc = [Poly(self.ringQBR, L, B, zero=False), Poly(self.ringQBR, L, B)]
        ringQBR.MulCoeffsMontgomery(test, xb, xb)
        ringQBR.AutomorphismNTT(xb, ringQBR.NthRoot() - GaloisGen, acc[0])
        self.BlindRotateCore(np.array(rows, dtype=np.uint64), acc, BRK)
        if not self.NTTFlag:
            for p in acc:
                ringQBR.INTT(p, p)
        res = {}
        for e, index in enumerate(slots):
            out = [Poly(self.ringQBR, L, 1, zero=False) for _ in range(2)]
            for o, p in zip(out, acc):
                o.CopyBatch(levelBR, 0, p, e, 1)
            res[index] = out
        return res
