"""The key-generation and key-switching protocols of the reference's multiparty package restated line for line over the oracle's
ring operations, the restated Encryptor (tests/encryptor_ref.py) and the samplers of tests/sampler_ref.py, as functions of byte-stream
sources: written from reading multiparty/keygen_cpk.go, keygen_evk.go, keygen_gal.go, keygen_relin.go, keyswitch_sk.go and
keyswitch_pk.go (file:line cited per step).  A polynomial is a uint64 array [limbs][N]; a secret
key a (Q, P) pair, NTT and Montgomery (P None without special primes); a CRP or a degree-0 share a dict q [rows][nQk][N],
p [rows][nPk][N] with its rows in the order of Value[i][j], i outer; a key the dict of tests/keygen_ref.py.  A protocol object
records each row's Gaussian (by row) and reads its source, whose position is the caller's to look at.  exp / log are injectable
as in sampler_ref."""
from __future__ import annotations

import math

import numpy as np

from oracle import oracle as O
from oracle import circuits as OC
from tests import keygen_ref as KR
from tests import sampler_ref as R


def _arr(pol):
    return np.array(pol, dtype=np.uint64)


def sample_crp(oQ, oP, crs: R.Source, levelQ, levelP, pw2=0):
    """sampleCRP (keygen_evk.go:64-83): us.ReadNew() for i outer, j inner -- a Read on the Q limbs, then one on the P limbs"""
    rows = KR.gadget_rows(oQ.moduli, levelQ, levelP, pw2)
    q = np.zeros((len(rows), levelQ + 1, oQ.N), dtype=np.uint64)
    p = np.zeros((len(rows), levelP + 1, oQ.N), dtype=np.uint64)
    for r in range(len(rows)):  # :74-80
        q[r] = _arr(R.uniform_read(crs, oQ.N, oQ.moduli[:levelQ + 1]))  # ringqp/samplers.go:47-55
        if levelP >= 0:
            p[r] = _arr(R.uniform_read(crs, oQ.N, oP.moduli[:levelP + 1]))
    return {"q": q, "p": p}


class EvaluationKeyGenProtocol:
    """one party: its Gaussian sampler reads `src`"""

    def __init__(self, oQ, oP, src: R.Source, sigma=3.2, bound=19.2, exp=math.exp, log=R._log):
        self.oQ, self.oP, self.src, self.sigma, self.bound, self.exp, self.log = oQ, oP, src, sigma, bound, exp, log
        self.gaussians = []  # per share generated: the Gaussian of each row (limbs of Q), by row
        self.operands = []   # per share generated: (skIn, skOut) as GenShare received them

    def gen_share(self, skIn, skOut, crp, levelQ, levelP, pw2=0):
        """GenShare (keygen_evk.go:86-183): skIn [>= levelQ + 1][N], skOut = (Q, P)"""
        oQ, oP, N = self.oQ, self.oP, self.oQ.N
        rows = KR.gadget_rows(oQ.moduli, levelQ, levelP, pw2)
        sizes = KR.base_two_sizes(oQ.moduli, levelQ, levelP, pw2)
        assert crp["q"].shape[0] == len(rows)  # :99-105
        has_p = levelP > -1
        if has_p:  # :114-116
            buffQ = oQ.MulScalarBigint(_arr(skIn)[:levelQ + 1], math.prod(oP.moduli[:levelP + 1]))
        else:  # :117-120
            levelP = 0
            buffQ = _arr(skIn)[:levelQ + 1].copy()
        mq = np.zeros((len(rows), levelQ + 1, N), dtype=np.uint64)
        mp = np.zeros((len(rows), levelP + 1 if has_p else 0, N), dtype=np.uint64)
        es = [None] * len(rows)
        for j in range(max(sizes)):  # :134
            for i in range(len(sizes)):  # :136
                if j < sizes[i]:  # :138
                    row = rows.index((i, j))
                    e = _arr(R.gaussian_read(self.src, N, oQ.moduli[:levelQ + 1], self.sigma, self.bound, False, exp=self.exp, log=self.log))  # :143
                    es[row] = e
                    cq = e
                    cp = OC.ExtendBasisSmallNormAndCenter(oQ, oP, cq, levelP) if has_p else None  # :145-147
                    cq = oQ.unop("MForm", oQ.NTTLazy(cq))  # :149-150
                    if has_p:
                        cp = oP.unop("MForm", oP.NTTLazy(cp))
                    for k in range(levelP + 1):  # :156-172
                        index = i * (levelP + 1) + k
                        if index >= levelQ + 1:  # :161
                            break
                        qi = np.uint64(oQ.moduli[index])
                        s = cq[index] + buffQ[index]
                        cq[index] = np.where(s >= qi, s - qi, s)  # CRed (:170)
                    mq[row] = oQ.binop("MulCoeffsMontgomeryThenSub", crp["q"][row], _arr(skOut[0])[:levelQ + 1], cq)  # :175
                    if has_p:
                        mp[row] = oP.binop("MulCoeffsMontgomeryThenSub", crp["p"][row], _arr(skOut[1])[:levelP + 1], cp)
            buffQ = oQ.scalarop("MulScalar", buffQ, 1 << pw2)  # :179
        self.gaussians.append(es)
        self.operands.append((skIn, skOut))
        return {"q": mq, "p": mp}

    def aggregate_shares(self, share1, share2):
        """AggregateShares (:186-215): ringQP.Add -- one CRed -- per row"""
        q = np.stack([self.oQ.binop("Add", a, b) for a, b in zip(share1["q"], share2["q"])])  # :210
        p = np.stack([self.oP.binop("Add", a, b) for a, b in zip(share1["p"], share2["p"])]) if share1["p"].shape[1] else share1["p"].copy()
        return {"q": q, "p": p}

    def gen_evaluation_key(self, share, crp, pw2=0, nj=None):
        """GenEvaluationKey (:218-241): Value[i][j] = (share, crp)"""
        return {"q": np.stack([share["q"], crp["q"]], axis=1), "p": np.stack([share["p"], crp["p"]], axis=1), "pw2": pw2, "nj": nj}


class GaloisKeyGenProtocol(EvaluationKeyGenProtocol):
    def gen_share(self, sk, galEl, crp, levelQ, levelP, pw2=0):
        """GenShare (keygen_gal.go:48-71)"""
        nth = self.oQ.NthRoot()
        galElInv = pow(int(galEl), nth - 1, nth)  # :57, ring.ModExp
        index = O.AutomorphismNTTIndex(self.oQ.N, nth, galElInv)  # ring.AutomorphismNTT (ring/automorphism.go)
        skOut = (self.oQ.AutomorphismNTTWithIndex(_arr(sk[0])[:levelQ + 1], index),  # :63
                 self.oP.AutomorphismNTTWithIndex(_arr(sk[1])[:levelP + 1], index) if levelP > -1 else None)  # :65-67
        return super().gen_share(sk[0], skOut, crp, levelQ, levelP, pw2)  # :69


def share_image(share):
    """the share as component 0 of he_evk_download gives it: [rows][nQk + nPk][N]"""
    return np.concatenate([share["q"], share["p"]], axis=1)


# ---- multiparty/keygen_relin.go -----------------------------------------------------------------------------------------------------------
class RelinearizationKeyGenProtocol:
    """one party: its ternary and Gaussian samplers read `src` (one PRNG for both, :38-52).  A share is a dict q [rows][comps][nQk][N],
    p [rows][comps][nPk][N], comps 2 for round one and 1 for round two"""

    def __init__(self, oQ, oP, src: R.Source, xs_p=2 / 3, sigma=3.2, bound=19.2, exp=math.exp, log=R._log):
        self.oQ, self.oP, self.src, self.xs_p, self.sigma, self.bound, self.exp, self.log = oQ, oP, src, xs_p, sigma, bound, exp, log
        self.gaussians = []  # per round generated: the Gaussians of each row, by row (round one: [e0, e1])

    def _gauss(self, levelQ):
        return _arr(R.gaussian_read(self.src, self.oQ.N, self.oQ.moduli[:levelQ + 1], self.sigma, self.bound, False, exp=self.exp, log=self.log))

    def _e_ntt(self, e, levelP, has_p):
        """sampler.Read; ExtendBasisSmallNormAndCenter; ringQP.NTT (:138-144)"""
        ep = OC.ExtendBasisSmallNormAndCenter(self.oQ, self.oP, e, levelP) if has_p else None
        return self.oQ.NTT(e), (self.oP.NTT(ep) if has_p else None)

    def gen_share_round_one(self, sk, crp, levelQ, levelP, pw2=0):
        """GenShareRoundOne (:91-184) -> (ephSk = (Q at the ring's top level, P), share)"""
        oQ, oP, N = self.oQ, self.oP, self.oQ.N
        rows = KR.gadget_rows(oQ.moduli, levelQ, levelP, pw2)
        sizes = KR.base_two_sizes(oQ.moduli, levelQ, levelP, pw2)
        has_p = levelP > -1
        skQ, skP = _arr(sk[0])[:levelQ + 1], (_arr(sk[1])[:levelP + 1] if has_p else None)
        if has_p:  # :105-107
            buffQ = oQ.MulScalarBigint(skQ, math.prod(oP.moduli[:levelP + 1]))
        else:  # :108-111
            levelP = 0
            buffQ = skQ.copy()
        buffQ = oQ.unop("IMForm", buffQ)  # :113
        # u (:116-121): the sampler stands at the parameters' top level; the rest runs at the share's levels
        uQ = _arr(R.ternary_read(self.src, N, oQ.moduli, self.xs_p, False))
        uP = OC.ExtendBasisSmallNormAndCenter(oQ, oP, uQ, levelP) if has_p else None
        uQ[:levelQ + 1] = oQ.unop("MForm", oQ.NTT(uQ[:levelQ + 1]))
        if has_p:
            uP = oP.unop("MForm", oP.NTT(uP))
        mq = np.zeros((len(rows), 2, levelQ + 1, N), dtype=np.uint64)
        mp = np.zeros((len(rows), 2, levelP + 1 if has_p else 0, N), dtype=np.uint64)
        es = [None] * len(rows)
        for j in range(max(sizes)):  # :133
            for i in range(len(sizes)):
                if j < sizes[i]:  # :136
                    row = rows.index((i, j))
                    e0 = self._gauss(levelQ)  # :138
                    hq, hp = self._e_ntt(e0, levelP, has_p)  # :140-144
                    for k in range(levelP + 1):  # :147-163
                        index = i * (levelP + 1) + k
                        if index >= levelQ + 1:
                            break
                        qi = np.uint64(oQ.moduli[index])
                        s = hq[index] + buffQ[index]
                        hq[index] = np.where(s >= qi, s - qi, s)
                    mq[row, 0] = oQ.binop("MulCoeffsMontgomeryThenSub", uQ[:levelQ + 1], crp["q"][row], hq)  # :166
                    if has_p:
                        mp[row, 0] = oP.binop("MulCoeffsMontgomeryThenSub", uP, crp["p"][row], hp)
                    e1 = self._gauss(levelQ)  # :170
                    hq, hp = self._e_ntt(e1, levelP, has_p)  # :172-176
                    mq[row, 1] = oQ.binop("MulCoeffsMontgomeryThenAdd", skQ, crp["q"][row], hq)  # :178
                    if has_p:
                        mp[row, 1] = oP.binop("MulCoeffsMontgomeryThenAdd", skP, crp["p"][row], hp)
                    es[row] = [e0, e1]
            buffQ = oQ.scalarop("MulScalar", buffQ, 1 << pw2)  # :182
        self.gaussians.append(es)
        return (uQ, uP), {"q": mq, "p": mp}

    def gen_share_round_two(self, ephSk, sk, round1, levelQ, levelP, pw2=0):
        """GenShareRoundTwo (:193-234)"""
        oQ, oP, N = self.oQ, self.oP, self.oQ.N
        rows = KR.gadget_rows(oQ.moduli, levelQ, levelP, pw2)
        has_p = levelP > -1
        skQ, skP = _arr(sk[0])[:levelQ + 1], (_arr(sk[1])[:levelP + 1] if has_p else None)
        dQ = oQ.binop("Sub", _arr(ephSk[0])[:levelQ + 1], skQ)  # :205
        dP = oP.binop("Sub", _arr(ephSk[1])[:levelP + 1], skP) if has_p else None
        mq = np.zeros((len(rows), 1, levelQ + 1, N), dtype=np.uint64)
        mp = np.zeros((len(rows), 1, levelP + 1 if has_p else 0, N), dtype=np.uint64)
        es = []
        for row in range(len(rows)):  # :211-212, i outer
            e = self._gauss(levelQ)  # :220
            es.append([e])
            eq, ep = self._e_ntt(e, levelP, has_p)  # :222-226
            t = oQ.binop("MulCoeffsMontgomeryLazy", round1["q"][row, 0], skQ)  # :217
            t = oQ.binop("Add", t, eq)  # :227
            mq[row, 0] = oQ.binop("MulCoeffsMontgomeryThenAdd", dQ, round1["q"][row, 1], t)  # :231
            if has_p:
                t = oP.binop("MulCoeffsMontgomeryLazy", round1["p"][row, 0], skP)
                t = oP.binop("Add", t, ep)
                mp[row, 0] = oP.binop("MulCoeffsMontgomeryThenAdd", dP, round1["p"][row, 1], t)
        self.gaussians.append(es)
        return {"q": mq, "p": mp}

    def aggregate_shares(self, share1, share2):
        """AggregateShares (:237-254): ringQP.Add on components 0..Degree()"""
        q = np.stack([[self.oQ.binop("Add", a, b) for a, b in zip(ra, rb)] for ra, rb in zip(share1["q"], share2["q"])])
        p = (np.stack([[self.oP.binop("Add", a, b) for a, b in zip(ra, rb)] for ra, rb in zip(share1["p"], share2["p"])])
             if share1["p"].shape[2] else share1["p"].copy())
        return {"q": q, "p": p}

    def gen_relinearization_key(self, round1, round2, pw2=0, nj=None):
        """GenRelinearizationKey (:261-276): MForm of round2[0] and of round1[1]"""
        q = np.stack([np.stack([self.oQ.unop("MForm", r2[0]), self.oQ.unop("MForm", r1[1])]) for r1, r2 in zip(round1["q"], round2["q"])])
        p = (np.stack([np.stack([self.oP.unop("MForm", r2[0]), self.oP.unop("MForm", r1[1])]) for r1, r2 in zip(round1["p"], round2["p"])])
             if round1["p"].shape[2] else np.zeros(q.shape[:2] + (0, q.shape[3]), dtype=np.uint64))
        return {"q": q, "p": p, "pw2": pw2, "nj": nj}


def gadget_image(share):
    """a share of any degree as he_evk_download gives its components: [rows][comps][nQk + nPk][N]"""
    return np.concatenate([share["q"], share["p"]], axis=2)


# ---- multiparty/keygen_cpk.go ------------------------------------------------------------------------------------------------------------
class PublicKeyGenProtocol:
    def __init__(self, oQ, oP, src: R.Source, sigma=3.2, bound=19.2, exp=math.exp, log=R._log):
        self.oQ, self.oP, self.src, self.sigma, self.bound, self.exp, self.log = oQ, oP, src, sigma, bound, exp, log
        self.gaussians = []

    def sample_crp(self, crs: R.Source):
        """SampleCRP (:56-60): one ringqp uniform Read at the top levels"""
        q = _arr(R.uniform_read(crs, self.oQ.N, self.oQ.moduli))
        return q, (_arr(R.uniform_read(crs, self.oQ.N, self.oP.moduli)) if self.oP is not None else None)

    def gen_share(self, sk, crp):
        """GenShare (:62-75)"""
        oQ, oP = self.oQ, self.oP
        e = _arr(R.gaussian_read(self.src, oQ.N, oQ.moduli, self.sigma, self.bound, False, exp=self.exp, log=self.log))  # :65
        self.gaussians.append(e)
        q = oQ.binop("MulCoeffsMontgomeryThenSub", sk[0], crp[0], oQ.unop("MForm", oQ.NTT(e)))  # :71-74
        p = None
        if oP is not None:  # :67-69
            ep = OC.ExtendBasisSmallNormAndCenter(oQ, oP, e, len(oP.moduli) - 1)
            p = oP.binop("MulCoeffsMontgomeryThenSub", sk[1], crp[1], oP.unop("MForm", oP.NTT(ep)))
        return q, p

    def aggregate_shares(self, a, b):  # :78-80
        return self.oQ.binop("Add", a[0], b[0]), (self.oP.binop("Add", a[1], b[1]) if self.oP is not None else None)


# ---- multiparty/keyswitch_sk.go ----------------------------------------------------------------------------------------------------------
def cks_noise(noise_fresh_sk: float, noise_sigma: float):
    """NewKeySwitchProtocol (:49-52)"""
    s = math.sqrt(noise_fresh_sk * noise_fresh_sk + noise_sigma * noise_sigma)
    return s, 6 * s


class KeySwitchProtocol:
    def __init__(self, oQ, src: R.Source, sigma, bound, exp=math.exp, log=R._log):
        self.oQ, self.src, self.sigma, self.bound, self.exp, self.log = oQ, src, sigma, bound, exp, log
        self.gaussians = []

    def gen_share(self, skIn, skOut, c1, level, is_ntt):
        """GenShare (:82-118): c1 = ct.Value[1] at `level`"""
        oQ, N = self.oQ, self.oQ.N
        delta = oQ.binop("Sub", _arr(skIn)[:level + 1], _arr(skOut)[:level + 1])  # :92
        c1 = _arr(c1)[:level + 1]
        c1ntt = c1 if is_ntt else oQ.NTTLazy(c1)  # :95-100
        share = oQ.binop("MulCoeffsMontgomeryLazy", c1ntt, delta)  # :103
        if not is_ntt:  # :105-108
            share = oQ.INTTLazy(share)
            before = [[int(w) for w in limb] for limb in share]
            share = _arr(R.gaussian_read(self.src, N, oQ.moduli[:level + 1], self.sigma, self.bound, False, before, exp=self.exp, log=self.log))
            self.gaussians.append(None)
        else:  # :110-114
            e = _arr(R.gaussian_read(self.src, N, oQ.moduli[:level + 1], self.sigma, self.bound, False, exp=self.exp, log=self.log))
            self.gaussians.append(e)
            share = oQ.binop("Add", share, oQ.NTT(e))
        return share


# ---- multiparty/keyswitch_pk.go ----------------------------------------------------------------------------------------------------------
class PublicKeySwitchProtocol:
    """one party: its rlwe.Encryptor reads enc_src, its noise sampler noise_src"""

    def __init__(self, oQ, oP, enc_src: R.Source, noise_src: R.Source, sigma, bound, xs_p=2 / 3, xe_sigma=3.2, xe_bound=19.2, exp=math.exp, log=R._log):
        from tests import encryptor_ref as ER
        self.oQ, self.oP, self.noise_src, self.sigma, self.bound, self.exp, self.log = oQ, oP, noise_src, sigma, bound, exp, log
        self.enc = ER.Encryptor(oQ, oP, enc_src, xs_p, xe_sigma, xe_bound, exp, log)

    def gen_share(self, sk, pk, c1, level, is_ntt, is_mont):
        """GenShare (:69-105): pk = ((pk0Q, pk0P), (pk1Q, pk1P)); -> (share0, share1)"""
        oQ, N = self.oQ, self.oQ.N
        if self.oP is not None:  # EncryptZero on a ring.Poly element (:77-88)
            ((s0, _), (s1, _)), = self.enc.encrypt_zero_pk([pk], level, 0, False, is_ntt, is_mont)
        else:
            ((s0, _), (s1, _)), = self.enc.encrypt_zero_pk_nop([pk], level, is_ntt)
        skQ, c1 = _arr(sk[0])[:level + 1], _arr(c1)[:level + 1]
        noise = lambda pol=None: _arr(R.gaussian_read(self.noise_src, N, oQ.moduli[:level + 1], self.sigma, self.bound, False, pol,
                                                      exp=self.exp, log=self.log))
        if is_ntt:  # :93-97
            s0 = oQ.binop("MulCoeffsMontgomeryThenAdd", c1, skQ, s0)
            s0 = oQ.binop("Add", s0, oQ.NTT(noise()))
        else:  # :98-103
            buff = oQ.INTT(oQ.binop("MulCoeffsMontgomeryLazy", oQ.NTTLazy(c1), skQ))
            buff = noise([[int(w) for w in limb] for limb in buff])
            s0 = oQ.binop("Add", s0, buff)
        return s0, s1
