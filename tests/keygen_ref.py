"""rlwe.KeyGenerator of the reference restated over the oracle's ring operations, the restated Encryptor (tests/encryptor_ref.py) and
the samplers of tests/sampler_ref.py, as functions of the byte stream: written from reading core/rlwe/keygenerator.go,
core/rlwe/gadgetciphertext.go:172-241, core/rlwe/utils.go:250-284 and ring/sampler_ternary.go:198-263 (file:line cited per step).
A polynomial is a uint64 array [limbs][N]; a secret key a (Q, P) pair, NTT and Montgomery (P None without special primes); an
evaluation key a dict q [rows][2][nQk][N], p [rows][2][nPk][N] with its rows in the order of evk.Value[i][j], i outer.
exp / log are injectable as in sampler_ref."""
from __future__ import annotations

import math

import numpy as np

from oracle import oracle as O
from tests import encryptor_ref as ER
from tests import sampler_ref as R


# ---- ring/sampler_ternary.go:198-263 ------------------------------------------------------------------------------------------------
class SparseTrace:
    def __init__(self):
        self.draws = self.rejected = 0


def sample_sparse(src: R.Source, N: int, moduli, hw: int, montgomery: bool, trace: SparseTrace | None = None):
    """TernarySampler.sampleSparse with f = (a, b, c) -> b (Read); the bytes come straight from the source"""
    tr = trace or SparseTrace()
    hw = min(hw, N)  # :202-204
    lut = R.matrix_values(moduli, montgomery)
    index = list(range(N))  # :211-214
    random_bytes = src.read((hw + 7) // 8)  # :216-222, ceil(hw / 8)
    pol = [[0] * N for _ in moduli]
    pointer = 0
    for i in range(hw):  # :228
        mask = (1 << (N - i).bit_length()) - 1  # :230
        while True:  # :232-236, randInt32: four bytes, big-endian
            j = int.from_bytes(src.read(4), "big") & mask
            tr.draws += 1
            if j < N - i:
                break
            tr.rejected += 1
        coeff = (random_bytes[0] >> (i & 7)) & 1  # :238
        idxj = index[j]
        for k in range(len(moduli)):  # :242-244
            pol[k][idxj] = lut[k][coeff + 1]
        index[j] = index[-1]  # :247-248
        index.pop()
        pointer += 1
        if pointer == 8:  # :252-255
            random_bytes = random_bytes[1:]
            pointer = 0
    for i in index:  # :258-262
        for k in range(len(moduli)):
            pol[k][i] = 0
    return pol


# ---- core/rlwe/params.go:523-550 ------------------------------------------------------------------------------------------------------
def base_rns_size(levelQ, levelP):
    return levelQ + 1 if levelP == -1 else (levelQ + levelP + 1) // (levelP + 1)


def base_two_sizes(moduliQ, levelQ, levelP, pw2):
    if pw2 == 0 or levelP > 0:
        return [1] * base_rns_size(levelQ, levelP)
    return [(int(round(math.log2(float(q)))) + pw2 - 1) // pw2 for q in moduliQ[:levelQ + 1]]


def gadget_rows(moduliQ, levelQ, levelP, pw2):
    """[(i, j)] in the order of evk.Value[i][j]"""
    return [(i, j) for i, n in enumerate(base_two_sizes(moduliQ, levelQ, levelP, pw2)) for j in range(n)]


# ---- core/rlwe/gadgetciphertext.go:172-241 -----------------------------------------------------------------------------------------------
def add_poly_times_gadget_vector(oQ, oP, pt, keys, levelQ, levelP, pw2):
    """keys: one or two arrays q [rows][2][levelQ + 1][N], changed in place: the term goes to component u of keys[u]"""
    assert 1 <= len(keys) <= 2  # :179
    moduli = oQ.moduli[:levelQ + 1]
    rows = gadget_rows(oQ.moduli, levelQ, levelP, pw2)
    sizes = base_two_sizes(oQ.moduli, levelQ, levelP, pw2)
    if levelP != -1:  # :183-188
        P = 1
        for p in oP.moduli[:levelP + 1]:
            P *= p
        buff = oQ.MulScalarBigint(np.asarray(pt)[:levelQ + 1], P)
    else:
        levelP = 0
        buff = np.array(pt, dtype=np.uint64)[:levelQ + 1].copy()
    for j in range(max(sizes)):  # :200
        for i in range(len(sizes)):
            if j < sizes[i]:
                row = rows.index((i, j))
                for k in range(levelP + 1):  # :213-231
                    index = i * (levelP + 1) + k
                    if index >= levelQ + 1:
                        break
                    qi = np.uint64(moduli[index])
                    for u, key in enumerate(keys):
                        s = key[row][u][index] + buff[index]
                        key[row][u][index] = np.where(s >= qi, s - qi, s)  # CRed
        buff = oQ.scalarop("MulScalar", buff, 1 << pw2)  # :237


# ---- core/rlwe/utils.go:250-284 -----------------------------------------------------------------------------------------------------------
def extend_ntt_montgomery(oQ, ringP, polQ, levelP):
    """ExtendBasisSmallNormAndCenterNTTMontgomery(rQ, rP.AtLevel(levelP), polQ, buff, polP) -> polP"""
    from oracle import oracle as _O
    r0 = _O.Ring(oQ.N, oQ.moduli[:1], oQ.conjugate_invariant)
    buff = r0.unop("IMForm", r0.INTT(np.asarray(polQ)[:1]))  # :256-257
    Q = oQ.moduli[0]
    out = np.empty((levelP + 1, oQ.N), dtype=np.uint64)
    c = buff[0]
    neg = c > np.uint64(Q >> 1)  # :271-275
    coeff = np.where(neg, np.uint64(Q) - c, c)
    for i, pi in enumerate(ringP.moduli[:levelP + 1]):  # :277-279
        out[i] = np.where(neg, np.uint64(pi) - coeff, coeff)
    rp = _O.Ring(oQ.N, ringP.moduli[:levelP + 1], oQ.conjugate_invariant)
    return rp.unop("MForm", rp.NTT(out))  # :282-283


# ---- core/rlwe/keygenerator.go --------------------------------------------------------------------------------------------------------------
class KeyGenerator:
    def __init__(self, oQ, oP, src: R.Source, xs_p=2 / 3, sigma=3.2, bound=19.2, exp=math.exp, log=R._log):
        self.oQ, self.oP, self.src, self.xs_p = oQ, oP, src, xs_p
        self.enc = ER.Encryptor(oQ, oP, src, xs_p, sigma, bound, exp, log)
        self.gaussians = []  # per key generated, per row: the Gaussian drawn (limbs of Q)
        self.operands = []   # per key generated: (skIn, skOut) as genEvaluationKey received them

    def _sk_from(self, q, levelQ, levelP):  # genSecretKeyFromSampler :58-70
        oQ, oP = self.oQ, self.oP
        q = np.array(q, dtype=np.uint64)
        p = None
        if levelP > -1:  # :64-66
            p = self.enc._lift(q, levelP)
        q = oQ.unop("MForm", oQ.NTT(q))  # :68-69
        if p is not None:
            p = oP.unop("MForm", oP.NTT(p))
        return q, p

    def gen_secret_key(self, levelQ, levelP):
        return self._sk_from(R.ternary_read(self.src, self.oQ.N, self.oQ.moduli[:levelQ + 1], self.xs_p, False), levelQ, levelP)  # :62

    def gen_secret_key_hw(self, hw, levelQ, levelP):  # :49-56
        return self._sk_from(sample_sparse(self.src, self.oQ.N, self.oQ.moduli[:levelQ + 1], hw, False), levelQ, levelP)

    def gen_evaluation_key(self, skIn, skOut, levelQ, levelP, pw2=0):
        """genEvaluationKey (:287-330): skIn [>= levelQ + 1][N], skOut = (Q, P)"""
        rows = gadget_rows(self.oQ.moduli, levelQ, levelP, pw2)
        q = np.zeros((len(rows), 2, levelQ + 1, self.oQ.N), dtype=np.uint64)
        p = np.zeros((len(rows), 2, levelP + 1, self.oQ.N), dtype=np.uint64)
        es = []
        for r in range(len(rows)):  # :309-320: one EncryptZero per row, IsNTT = IsMontgomery = true
            n0 = len(self.enc.drawn)
            ((c0Q, c0P), (c1Q, c1P)), = self.enc.encrypt_zero_sk([skOut], levelQ, levelP, 1, 1)
            es.append(self.enc.drawn[n0])
            q[r, 0], q[r, 1] = c0Q, c1Q
            if levelP >= 0:
                p[r, 0], p[r, 1] = c0P, c1P
        self.gaussians.append(es)
        self.operands.append((skIn, skOut))
        add_poly_times_gadget_vector(self.oQ, self.oP, skIn, [q], levelQ, levelP, pw2)  # :326
        return {"q": q, "p": p, "pw2": pw2, "nj": base_two_sizes(self.oQ.moduli, levelQ, levelP, pw2) if pw2 else None}

    def gen_evaluation_key_sk(self, skInQ, skOutQ, levelQ, levelP, pw2=0):
        """GenEvaluationKey (:261-285): the Q parts of two secret keys, each of any degree up to N and of any level"""
        oQ, N = self.oQ, self.oQ.N
        small_to_large = lambda pol: np.repeat(np.asarray(pol, dtype=np.uint64)[:len(oQ.moduli)], N // pol.shape[1], axis=1)  # ring/operations.go:380-392
        outQ = small_to_large(skOutQ)  # :271
        lout = outQ.shape[0] - 1
        assert lout >= levelQ  # (below, genEvaluationKey reads limbs of the pooled buffer that this call never wrote)
        outP = extend_ntt_montgomery(oQ, self.oP, outQ, levelP) if levelP != -1 else None  # :276-278
        skIn = small_to_large(skInQ)  # :281
        skIn = extend_ntt_montgomery(oQ, oQ, skIn, lout)  # :282: every limb 0..lout from limb 0
        return self.gen_evaluation_key(skIn, (outQ, outP), levelQ, levelP, pw2)  # :284

    def gen_relinearization_key(self, sk, levelQ, levelP, pw2=0):  # :113-120
        skQ = sk[0][:levelQ + 1]
        return self.gen_evaluation_key(self.oQ.binop("MulCoeffsMontgomery", skQ, skQ), sk, levelQ, levelP, pw2)

    def gen_galois_key(self, galEl, sk, levelQ, levelP, pw2=0):  # :140-177
        nth = self.oQ.NthRoot()
        index = O.AutomorphismNTTIndex(self.oQ.N, nth, pow(int(galEl), -1, nth))  # :157-159
        skOut = (self.oQ.AutomorphismNTTWithIndex(sk[0][:levelQ + 1], index),  # :167
                 self.oP.AutomorphismNTTWithIndex(sk[1][:levelP + 1], index) if levelP >= 0 else None)  # :169-171
        return self.gen_evaluation_key(sk[0], skOut, levelQ, levelP, pw2)  # :173

    def gen_galois_keys(self, galEls, sk, levelQ, levelP, pw2=0):  # :182-196
        return [self.gen_galois_key(g, sk, levelQ, levelP, pw2) for g in galEls]


def image(key):
    """the key as he_evk_download gives it: [rows][2][nQk + nPk][N]"""
    return np.concatenate([key["q"], key["p"]], axis=2)
