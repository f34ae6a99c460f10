"""rlwe.Encryptor and rlwe.Decryptor of the reference restated over the oracle's ring operations (oracle.Ring / BasisExtender) and
the samplers of tests/sampler_ref.py, as functions of the byte stream: written from reading core/rlwe/encryptor.go and
core/rlwe/decryptor.go (file:line cited per step).  A polynomial is a uint64 array [limbs][N]; a QP polynomial a (Q, P) pair.

A batch of B ciphertexts is a list of B entries.  Each draw of a call is made for every entry before the next step of the call
(include/hering_encryptor.h), which for B = 1 is the reference's order exactly.  exp / log are injectable as in sampler_ref."""
from __future__ import annotations

import math

import numpy as np

from oracle import circuits as OC
from tests import sampler_ref as R


def _arr(pol):
    return np.array(pol, dtype=np.uint64)


class Encryptor:
    def __init__(self, oQ, oP, src: R.Source, xs_p=2 / 3, sigma=3.2, bound=19.2, exp=math.exp, log=R._log):
        """oP None: no special primes"""
        self.oQ, self.oP, self.src, self.xs_p, self.sigma, self.bound, self.exp, self.log = oQ, oP, src, xs_p, sigma, bound, exp, log
        if oP is not None:
            from oracle import oracle as O
            self.be = O.BasisExtender(oQ, oP)
        self.drawn = []  # the small polynomials drawn, in order (tests read the Gaussians back)

    # -- the samplers NewEncryptor builds (:50-76): montgomery = false
    def _gauss(self, levelQ, pol=None):
        out = _arr(R.gaussian_read(self.src, self.oQ.N, self.oQ.moduli[:levelQ + 1], self.sigma, self.bound, False,
                                   None if pol is None else [[int(w) for w in limb] for limb in pol], exp=self.exp, log=self.log))
        return out

    def _ternary(self, levelQ):
        return _arr(R.ternary_read(self.src, self.oQ.N, self.oQ.moduli[:levelQ + 1], self.xs_p, False))

    def _uniform(self, levelQ, levelP):
        q = _arr(R.uniform_read(self.src, self.oQ.N, self.oQ.moduli[:levelQ + 1]))
        p = _arr(R.uniform_read(self.src, self.oQ.N, self.oP.moduli[:levelP + 1])) if levelP >= 0 else None
        return q, p

    def _lift(self, q, levelP):  # ringqp.Ring.ExtendBasisSmallNormAndCenter (ring/ringqp/operations.go:325)
        return OC.ExtendBasisSmallNormAndCenter(self.oQ, self.oP, q, levelP)

    # -- encryptZeroSk (:347-393) + encryptZeroSkFromC1QP (:406-433); sk = [(skQ, skP)] per entry; levelP = -1: the ring.Poly form
    def encrypt_zero_sk(self, sk, levelQ, levelP, is_ntt, is_mont, batch=1):
        oQ, oP = self.oQ, self.oP
        c1 = [self._uniform(levelQ, levelP) for _ in range(batch)]  # :361 / :383
        if not is_ntt:  # :363-365 / :385-387
            c1 = [(oQ.NTT(q), oP.NTT(p) if levelP >= 0 else None) for q, p in c1]
        e = [self._gauss(levelQ) for _ in range(batch)]  # :411
        self.drawn += e
        out = []
        for b in range(batch):
            skQ, skP = sk[b]
            c0Q = e[b]
            c0P = self._lift(c0Q, levelP) if levelP >= 0 else None  # :412-414
            c0Q = oQ.NTT(c0Q)  # :416
            if levelP >= 0:
                c0P = oP.NTT(c0P)
            if is_mont:  # :420-422
                c0Q = oQ.unop("MForm", c0Q)
                if levelP >= 0:
                    c0P = oP.unop("MForm", c0P)
            c1Q, c1P = c1[b]
            c0Q = oQ.binop("MulCoeffsMontgomeryThenSub", c1Q, skQ[:levelQ + 1], c0Q)  # :425
            if levelP >= 0:
                c0P = oP.binop("MulCoeffsMontgomeryThenSub", c1P, skP[:levelP + 1], c0P)
            if not is_ntt:  # :427-430
                c0Q, c1Q = oQ.INTT(c0Q), oQ.INTT(c1Q)
                if levelP >= 0:
                    c0P, c1P = oP.INTT(c0P), oP.INTT(c1P)
            out.append(((c0Q, c0P), (c1Q, c1P)))
        return out

    # -- encryptZeroPk (:204-299); pk = [((pk0Q, pk0P), (pk1Q, pk1P))] per entry; qp False: the ring.Poly element (levelP = 0, :217)
    def encrypt_zero_pk(self, pk, levelQ, levelP, qp, is_ntt, is_mont, batch=1):
        oQ, oP = self.oQ, self.oP
        if not qp:
            levelP = 0
        u = [self._ternary(levelQ) for _ in range(batch)]  # :242
        e0 = [self._gauss(levelQ) for _ in range(batch)]  # :259
        e1 = [self._gauss(levelQ) for _ in range(batch)]  # :263
        self.drawn += u + e0 + e1
        out = []
        for b in range(batch):
            uQ, uP = oQ.NTT(u[b]), oP.NTT(self._lift(u[b], levelP))  # :243-246
            ct = []
            for k, e in enumerate((e0[b], e1[b])):
                pkQ, pkP = pk[b][k]
                cQ = oQ.INTT(oQ.binop("MulCoeffsMontgomery", uQ, pkQ[:levelQ + 1]))  # :250-255
                cP = oP.INTT(oP.binop("MulCoeffsMontgomery", uP, pkP[:levelP + 1]))
                cQ = oQ.binop("Add", cQ, e)  # :259-265
                cP = oP.binop("Add", cP, self._lift(e, levelP))
                if not qp:
                    cQ = self.be.ModDownQPtoQ(levelQ, levelP, cQ, cP)  # :271-274
                    cP = None
                if is_ntt:  # :276-279 / :287-290
                    cQ = oQ.NTT(cQ)
                    cP = oP.NTT(cP) if qp else None
                if is_mont:  # :281-284 / :292-295
                    cQ = oQ.unop("MForm", cQ)
                    cP = oP.unop("MForm", cP) if qp else None
                ct.append((cQ, cP))
            out.append(tuple(ct))
        return out

    # -- encryptZeroPkNoP (:301-342)
    def encrypt_zero_pk_nop(self, pk, levelQ, is_ntt, batch=1):
        oQ = self.oQ
        u = [self._ternary(levelQ) for _ in range(batch)]  # :310
        self.drawn += u
        u = [oQ.NTT(x) for x in u]  # :311
        ct = [[oQ.binop("MulCoeffsMontgomery", u[b], pk[b][k][0][:levelQ + 1]) for k in range(2)] for b in range(batch)]  # :316-318
        for k in range(2):  # :321-339
            for b in range(batch):
                if is_ntt:
                    e = self._gauss(levelQ)
                    self.drawn.append(e)
                    ct[b][k] = oQ.binop("Add", ct[b][k], oQ.NTT(e))
                else:
                    ct[b][k] = self._gauss(levelQ, oQ.INTT(ct[b][k]))  # ReadAndAdd
        return [((c[0], None), (c[1], None)) for c in ct]

    # -- addPtToCt (:481-507)
    def add_pt_to_ct(self, level, pt, pt_is_ntt, c0, ct_is_ntt):
        oQ = self.oQ
        buff = pt[:level + 1]
        if pt_is_ntt and not ct_is_ntt:
            buff = oQ.NTT(buff)  # :493
        elif not pt_is_ntt and ct_is_ntt:
            buff = oQ.INTT(buff)  # :500
        return oQ.binop("Add", c0[:level + 1], buff)  # :506


def decrypt(oQ, skQ, ct, ct_level, pt_level, is_ntt, reduce_always=False):
    """Decryptor.Decrypt (decryptor.go:51-93): ct = [c0, c1, ...]; returns (pt words on limbs 0..level, level).  reduce_always: the
    Reduce of :86 whatever the degree -- the device's form for a coefficient-domain ciphertext of degree 7 mod 8, where the
    reference's INTT reads unreduced sums of NTTLazy words (up to 7q) and is not exact (include/hering_encryptor.h)"""
    level = min(ct_level, pt_level)  # :53
    degree = len(ct) - 1
    sk = skQ[:level + 1]
    pt = ct[degree][:level + 1].copy() if is_ntt else oQ.NTTLazy(ct[degree][:level + 1])  # :61-65
    for i in range(degree, 0, -1):  # :67
        pt = oQ.binop("MulCoeffsMontgomery", pt, sk)  # :69
        pt = oQ.binop("Add", pt, ct[i - 1][:level + 1] if is_ntt else oQ.NTTLazy(ct[i - 1][:level + 1]))  # :71-79
        if i & 7 == 7:  # :81
            pt = oQ.unop("Reduce", pt)
    if degree & 7 != 7 or reduce_always:  # :86
        pt = oQ.unop("Reduce", pt)
    if not is_ntt:  # :90
        pt = oQ.INTT(pt)
    return pt, level
