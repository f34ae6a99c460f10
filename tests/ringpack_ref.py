"""core/rlwe/ring_packing.go restated over oracle.Ring / oracle.Evaluator, statement for statement (test infrastructure: the
reference the device entries of include/hering_ringpack.h and lattigo_amd.rlwe.RingPackingEvaluator are compared with).

It uses MATERIALISED monomial tables, built the way GenXPow2NTT builds them (a monomial, one NTT, repeated squaring), so it does
not depend on the identity the device kernels rest on (the tables as views of the twiddle tables).

A ciphertext is a numpy array [2][level + 1][N] in the NTT domain; a map of ciphertexts is a dict {index: array}.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O

GaloisGen = 5


def GenXPow2NTT(r: O.Ring, logN: int, div: bool):
    """ring_packing.go:772-810"""
    xPow = [None] * logN
    for i in range(logN):
        idx = 1 << i
        if div:
            idx = r.N - idx                                                        # :786-788
        if i == 0:
            p = r.NewPoly()
            for j, q in enumerate(r.moduli):
                p[j, idx] = O.MForm(1, q)                                          # :794-796
            xPow[i] = r.NTT(p)                                                     # :798
        else:
            xPow[i] = r.binop("MulCoeffsMontgomery", xPow[i - 1], xPow[i - 1])     # :801
    if div:
        xPow[0] = r.unop("Neg", xPow[0])                                           # :805-807
    return xPow


def getMinimumGap(lst):
    """ring_packing.go:812-845; returns (gap, logGap) as the reference (gap = the odd part)"""
    gap, logGap = 0x7FFFFFFFFFFFFFFF, 0
    for i in range(1, len(lst)):
        a, b = lst[i - 1], lst[i]
        if a > b:
            raise ValueError("invalid index list: element must be sorted from smallest to largest")
        if a == b:
            raise ValueError("invalid index list: contains duplicated elements")
        gap = min(gap, b - a)
        if gap == 1:
            break
    while gap & 1 == 0:
        logGap += 1
        gap >>= 1
    return gap, logGap


def GaloisElementsForExpand(N: int, logN: int):
    """ring_packing_keys.go:143-153"""
    return [(2 * N) // (2 << i) + 1 for i in range(logN)]


def GaloisElementsForPack(N: int, logGap: int):
    """ring_packing_keys.go:156-180 (standard ring)"""
    logN = N.bit_length() - 1
    assert 0 <= logGap <= logN
    g = [pow(GaloisGen, 1 << i, 2 * N) for i in range(logGap)]
    if logGap == logN:
        g.append(2 * N - 1)
    return g


def switch_down_ntt(a, rLarge: O.Ring, n: int):
    """SwitchCiphertextRingDegreeNTT, N -> n, one polynomial (core/rlwe/element.go:260-279)"""
    q = rLarge.moduli[: a.shape[0]]
    return O.Ring(n, q).NTT(O.Ring(rLarge.N, q).INTT(a)[:, :: rLarge.N // n].copy())


def switch_up_ntt(a, gap: int):
    """ring.MapSmallDimensionToLargerDimensionNTT (ring/operations.go:380)"""
    return np.repeat(a, gap, axis=1)


class RingPackingEvaluator:
    """ring_packing.go:13-50.  rings: {logN: (O.Ring Q, O.Ring P)} with the same moduli at every degree; RingSwitchingKeys:
    {(logN_from, logN_to): O.EvaluationKey}; ExtractKeys / RepackKeys: {logN: {galEl: O.EvaluationKey}}."""

    def __init__(self, rings, RingSwitchingKeys=None, ExtractKeys=None, RepackKeys=None):
        self.rings = rings
        self.RingSwitchingKeys = RingSwitchingKeys or {}
        self.ExtractKeys, self.RepackKeys = ExtractKeys, RepackKeys
        self.Evaluators = {n: O.Evaluator(q, p) for n, (q, p) in rings.items()}    # :39
        self.XPow2NTT = {n: GenXPow2NTT(q, n, False) for n, (q, _) in rings.items()}     # :40
        self.XInvPow2NTT = {n: GenXPow2NTT(q, n, True) for n, (q, _) in rings.items()}   # :41

    def MinLogN(self):
        return min(self.rings)

    def MaxLogN(self):
        return max(self.rings)

    def ringQ(self, logN, level):
        q = self.rings[logN][0]
        return O.Ring(q.N, q.moduli[: level + 1])

    # rlwe.Evaluator.ApplyEvaluationKey at the evaluator's degree (evaluator_evaluationkey.go:98-106)
    def _apply(self, logN, ct, evk):
        level = ct.shape[1] - 1
        gp = self.Evaluators[logN].GadgetProduct(level, ct[1], evk)
        return np.stack([self.ringQ(logN, level).binop("Add", ct[0], gp[0]), gp[1]])

    def _automorphism(self, logN, ct, galEl, keys):
        return self.Evaluators[logN].Automorphism(ct, int(galEl), keys[int(galEl)])

    # ---- Split (:173-228): returns (ctEvenNHalf, ctOddNHalf or None)
    def Split(self, ctN, odd=True):
        if self.MinLogN() == self.MaxLogN():
            raise ValueError("method is not supported when eval.MinLogN() == eval.MaxLogN()")
        LogN = ctN.shape[2].bit_length() - 1
        if LogN <= self.MinLogN():
            raise ValueError("ctN.Log() must be greater than eval.MinLogN()")
        level = ctN.shape[1] - 1
        ctTmp = self._apply(LogN, ctN, self.RingSwitchingKeys[(LogN, LogN - 1)])   # :201
        r = self.ringQ(LogN, level)                                                # :205
        n = r.N // 2
        even = np.stack([switch_down_ntt(ctTmp[k], r, n) for k in range(2)])       # :210
        if not odd:
            return even, None
        x = self.XInvPow2NTT[LogN][0][: level + 1]
        ctTmp = np.stack([r.binop("MulCoeffsMontgomery", ctTmp[k], x) for k in range(2)])  # :221-222
        return even, np.stack([switch_down_ntt(ctTmp[k], r, n) for k in range(2)])          # :223

    # ---- Merge (:376-426)
    def Merge(self, ctEvenNHalf, ctOddNHalf):
        if self.MinLogN() == self.MaxLogN():
            raise ValueError("method is not supported when eval.MinLogN() == eval.MaxLogN()")
        if ctEvenNHalf is None:
            raise ValueError("ctEvenNHalf cannot be nil")
        LogN = ctEvenNHalf.shape[2].bit_length()
        if LogN - 1 >= self.MaxLogN():
            raise ValueError("ctEvenNHalf.LogN() must be smaller than eval.MaxLogN()")
        level = ctEvenNHalf.shape[1] - 1
        r = self.ringQ(LogN, level)
        ctN = np.stack([switch_up_ntt(ctEvenNHalf[k], 2) for k in range(2)])       # :411
        if ctOddNHalf is not None:
            x = self.XPow2NTT[LogN][0][: level + 1]
            ctTmp = [switch_up_ntt(ctOddNHalf[k], 2) for k in range(2)]            # :414
            ctN = np.stack([r.binop("MulCoeffsMontgomeryThenAdd", ctTmp[k], x, ctN[k]) for k in range(2)])  # :415-416
        return self._apply(LogN, ctN, self.RingSwitchingKeys[(LogN - 1, LogN)])    # :420

    # ---- Expand (:448-571), NTT-domain input
    def Expand(self, ct, logGap):
        logN = ct.shape[2].bit_length() - 1
        level = ct.shape[1] - 1
        if self.ExtractKeys is None or logN not in self.ExtractKeys:
            raise ValueError("eval.ExtractKeys[%d] is nil" % logN)
        evk = self.ExtractKeys[logN]
        xPow2 = self.XInvPow2NTT[logN]
        ringQ = self.ringQ(logN, level)
        NInv = pow(1 << logN, -1, int(np.prod([int(q) for q in ringQ.moduli], dtype=object)))  # :506-507
        cts = {0: np.stack([ringQ.MulScalarBigint(ct[k], NInv) for k in range(2)])}             # :509-510
        gap = 1 << logGap
        for i in range(logN):
            n = 1 << i
            galEl = ringQ.N // n + 1                                               # :524
            for j in range(0, n, gap):
                c0 = cts[j]
                tmp = self._automorphism(logN, c0, galEl, evk)                     # :532
                if j + n // gap > 0:
                    c1 = c0.copy()                                                 # :538
                    c0 = np.stack([ringQ.binop("Add", c0[k], tmp[k]) for k in range(2)])      # :541-542
                    c1 = np.stack([ringQ.binop("Sub", c1[k], tmp[k]) for k in range(2)])      # :545-546
                    c1 = np.stack([ringQ.binop("MulCoeffsMontgomery", c1[k], xPow2[i][: level + 1]) for k in range(2)])  # :549-550
                    cts[j], cts[j + n] = c0, c1
                else:
                    cts[j] = np.stack([ringQ.binop("Add", c0[k], tmp[k]) for k in range(2)])  # :557-558
        return cts

    # ---- Pack (:573-770); cts: {index: ciphertext}, consumed
    def Pack(self, cts, inputLogGap, zeroGarbageSlots):
        if len(cts) == 0:
            raise ValueError("len(cts) = 0")
        cts = dict(cts)
        keys = sorted(cts)
        logN = cts[keys[0]].shape[2].bit_length() - 1
        level = cts[keys[0]].shape[1] - 1
        if self.RepackKeys is None or logN not in self.RepackKeys:
            raise ValueError("eval.RepackKeys[%d] is nil" % logN)
        evk = self.RepackKeys[logN]
        xPow2 = self.XPow2NTT[logN]
        N = 1 << logN
        if len(keys) > 1:
            gap, logGap = getMinimumGap(keys)                                      # :642
        else:
            gap, logGap = N, logN
        ringQ = self.ringQ(logN, level)
        logStart, logEnd = logN - inputLogGap, logN
        if not zeroGarbageSlots and gap > 0:
            logEnd -= logGap                                                       # :655-659
        if logStart >= logEnd:
            raise ValueError("gaps between ciphertexts is smaller than inputLogGap > N")
        NInv = pow(1 << (logEnd - logStart), -1, int(np.prod([int(q) for q in ringQ.moduli], dtype=object)))  # :665-666
        for key in keys:
            cts[key] = np.stack([ringQ.MulScalarBigint(cts[key][k], NInv) for k in range(2)])  # :682-683
        add = lambda a, b: np.stack([ringQ.binop("Add", a[k], b[k]) for k in range(2)])
        sub = lambda a, b: np.stack([ringQ.binop("Sub", a[k], b[k]) for k in range(2)])
        for i in range(logStart, logEnd):
            t = 1 << (logN - 1 - i)
            x = xPow2[len(xPow2) - i - 1][: level + 1]
            galEl = 2 * N - 1 if i == 0 else pow(GaloisGen, 1 << (i - 1), 2 * N)   # :728-732
            for jx in range(t):
                jy = jx + t
                a, b = cts.get(jx), cts.get(jy)
                tmpa = None
                if b is not None:
                    b = np.stack([ringQ.binop("MulCoeffsMontgomery", b[k], x) for k in range(2)])  # :703-704
                    if a is not None:
                        tmpa = sub(a, b)                                           # :709-710
                        a = add(a, b)                                              # :713-714
                    else:
                        cts[jx] = b                                                # :718
                    cts.pop(jy, None)                                              # :721
                if a is not None:
                    src = tmpa if b is not None else a
                    tmpa = self._automorphism(logN, src, galEl, evk)               # :734-742
                    cts[jx] = add(a, tmpa)                                         # :745-746
                elif b is not None:
                    tmpa = self._automorphism(logN, b, galEl, evk)                 # :758
                    cts[jx] = sub(b, tmpa)                                         # :763-764
        return cts[0]

    # ---- extract (:72-171); idx: an iterable of indices
    def extract(self, ct, idx, naive):
        logNMax = ct.shape[2].bit_length() - 1
        logNMin = self.MinLogN()
        level = ct.shape[1] - 1
        logNFactor = logNMax - logNMin
        NFactor = 1 << logNFactor
        keys = sorted(idx)
        _, logGap = getMinimumGap(keys)                                            # :83
        tmpCts = {0: ct.copy()}
        for i in range(logNFactor):
            t = 1 << i
            logGap = max(0, logGap - 1)                                            # :97
            for j in range(t):
                if tmpCts.get(j) is not None:
                    tmpCts[j], tmpCts[j + t] = self.Split(tmpCts[j])               # :106-111
        buckets = {}
        for i in keys:
            buckets.setdefault(i & (NFactor - 1), []).append(i // NFactor)         # :121-124
        cts = {}
        for i in buckets:
            if naive:
                ciphertexts = {j: tmpCts[i].copy() for j in buckets[i]}            # :134-136
                XInv = self.XInvPow2NTT[logNMin]
                ringQ = self.ringQ(logNMin, level)
                for b in range(logNMin):
                    for j in ciphertexts:
                        if (j >> b) & 1:
                            ciphertexts[j] = np.stack([ringQ.binop("MulCoeffsMontgomery", ciphertexts[j][k], XInv[b][: level + 1])
                                                       for k in range(2)])         # :148-149
            else:
                ciphertexts = self.Expand(tmpCts[i], logGap)                       # :155
            for j in buckets[i]:
                if j not in ciphertexts:
                    raise ValueError("invalid ciphertexts map")
                cts[i + j * NFactor] = ciphertexts[j]                              # :162
        return cts

    def Extract(self, ct, idx):
        return self.extract(ct, idx, False)

    def ExtractNaive(self, ct, idx):
        return self.extract(ct, idx, True)

    # ---- repack (:273-374)
    def repack(self, cts, naive):
        keys = sorted(cts)
        logNMin = cts[keys[0]].shape[2].bit_length() - 1
        logNMax = self.MaxLogN()
        level = cts[keys[0]].shape[1] - 1
        logNFactor = logNMax - logNMin
        NFactor = 1 << logNFactor
        ctsSmallN = [dict() for _ in range(NFactor)]
        for i in keys:
            ctsSmallN[i & (NFactor - 1)][i // NFactor] = cts[i]                    # :294-296
        ctsLargeN = {}
        for i in range(NFactor):
            if naive:
                tmpCts = ctsSmallN[i]
                XPow2 = self.XPow2NTT[logNMin]
                ringQ = self.ringQ(logNMin, level)
                for l in range(logNMin):
                    t = 1 << (logNMin - 1 - l)
                    x = XPow2[len(XPow2) - l - 1][: level + 1]
                    for jx in range(t):
                        jy = jx + t
                        a, b = tmpCts.get(jx), tmpCts.get(jy)
                        if b is not None:
                            b = np.stack([ringQ.binop("MulCoeffsMontgomery", b[k], x) for k in range(2)])   # :324-325
                            if a is not None:
                                tmpCts[jx] = np.stack([ringQ.binop("Add", a[k], b[k]) for k in range(2)])   # :329-330
                            else:
                                tmpCts[jx] = b                                     # :334
                            tmpCts.pop(jy, None)                                   # :337
                ctsLargeN[i] = tmpCts.get(0)                                       # :342
            elif len(ctsSmallN[i]) != 0:
                ctsLargeN[i] = self.Pack(ctsSmallN[i], logNMin, True)              # :346
        for i in range(logNFactor - 1, -1, -1):
            t = 1 << i
            for j in range(t):
                if ctsLargeN.get(j) is not None or ctsLargeN.get(j + 1) is not None:   # :359
                    ctsLargeN[j] = self.Merge(ctsLargeN.get(j), ctsLargeN.get(j + t))  # :363-367
                    ctsLargeN[j + t] = None                                            # :368
        return ctsLargeN.get(0)

    def Repack(self, cts):
        return self.repack(cts, False)

    def RepackNaive(self, cts):
        return self.repack(cts, True)


# ---- keys and plaintexts of the reference's own test (ring_packing_keys.go:59-139, ring_packing_test.go) with tests/rlwe_fixtures ----
def gen_test_keys(rng, logNMax, logNMin, q, p, extract_at=(), repack_at=()):
    """Ternary secrets per degree chained by ring-switching keys (GenRingSwitchingKeys, :59-115), Galois keys for Expand at the
    degrees of `extract_at` and for Pack at those of `repack_at` (:119-139).  Returns (rings, sk, RingSwitchingKeys, ExtractKeys,
    RepackKeys) with O.EvaluationKey values."""
    from tests.rlwe_fixtures import SecretKey, gen_evaluation_key, gen_galois_keys
    rings = {n: (O.Ring(1 << n, q), O.Ring(1 << n, p)) for n in range(logNMin, logNMax + 1)}
    sk = {n: SecretKey(rng, *rings[n]) for n in rings}
    rsk = {}
    for i in range(logNMin, logNMax):
        up = np.zeros(2 << i, dtype=np.int64)
        up[::2] = sk[i].vals  # the small secret in the large ring: s(Y), Y = X^2
        sk_up = SecretKey(rng, *rings[i + 1], vals=up)
        rsk[(i, i + 1)] = gen_evaluation_key(rng, *rings[i + 1], sk_up.Q, sk[i + 1])
        rsk[(i + 1, i)] = gen_evaluation_key(rng, *rings[i + 1], sk[i + 1].Q, sk_up)
    ext = {n: gen_galois_keys(rng, *rings[n], sk[n], GaloisElementsForExpand(1 << n, n)) for n in extract_at}
    rep = {n: gen_galois_keys(rng, *rings[n], sk[n], GaloisElementsForPack(1 << n, n)) for n in repack_at}
    return rings, sk, rsk, ext, rep


def gen_plaintext(N, maxv=1 << 40):
    """genPlaintextNTT's coefficients (ring_packing_test.go:489-508): c[j] = floor(j * max / N)"""
    return np.array([int(float(j) * (float(maxv) / float(N))) for j in range(N)], dtype=np.int64)


def encrypt(rng, ringQ: O.Ring, skQ, coeffs, sigma=3.2):
    """(-a s + e + m, a) in the NTT domain at the ring's level"""
    from tests.rlwe_fixtures import small_to_rns
    N = ringQ.N
    a = np.stack([rng.integers(0, int(x), size=N, dtype=np.uint64) for x in ringQ.moduli])
    e = np.clip(np.rint(rng.normal(0.0, sigma, size=N)), -19, 19).astype(np.int64)
    m = ringQ.NTT(small_to_rns(np.asarray(coeffs, dtype=np.int64) + e, ringQ.moduli))
    return np.stack([ringQ.binop("Sub", m, ringQ.binop("MulCoeffsMontgomery", a, skQ[: len(ringQ.moduli)])), a])


def decrypt_centered(ringQ: O.Ring, ct, skQ):
    """the centred coefficients of limb 0 of the decryption (one modulus carries the whole value at the test's parameters)"""
    from tests.rlwe_fixtures import phase
    c = ringQ.INTT(phase(ringQ, ct, skQ))[0]
    q0 = int(ringQ.moduli[0])
    return np.array([int(x) - q0 if int(x) > q0 // 2 else int(x) for x in c], dtype=object)


def log2_std(v):
    """ring.Ring.Log2OfStandardDeviation of centred values"""
    s = float(np.std(np.array(v, dtype=np.float64)))
    return float(np.log2(s)) if s > 0 else 0.0
