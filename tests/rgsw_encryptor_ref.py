"""rgsw.Encryptor and blindrot.GenEvaluationKeyNew of the reference restated over the restated rlwe.Encryptor (tests/encryptor_ref.py),
the gadget term and the Galois keys of tests/keygen_ref.py and the samplers of tests/sampler_ref.py, as functions of the byte
stream: written from reading core/rgsw/encryptor.go and core/rgsw/blindrot/keys.go:46-108 (file:line cited per step).  An RGSW
ciphertext is a pair of keys in the form of keygen_ref (q [rows][2][nQk][N], p [rows][2][nPk][N], rows in the order of
Value[i][j], i outer).  exp / log are injectable as in sampler_ref."""
from __future__ import annotations

import math

import numpy as np

from oracle import oracle as O
from tests import encryptor_ref as ER
from tests import keygen_ref as KR
from tests import sampler_ref as R

WINDOW_SIZE = 10  # keys.go:14
GALOIS_GEN = 5


class _RlweEncryptor(ER.Encryptor):
    """the embedded *rlwe.Encryptor, recording the position of the source after every draw"""

    def __init__(self, *a):
        super().__init__(*a)
        self.positions = []

    def _uniform(self, levelQ, levelP):
        out = super()._uniform(levelQ, levelP)
        self.positions.append(self.src.pos)
        return out

    def _gauss(self, levelQ, pol=None):
        out = super()._gauss(levelQ, pol)
        self.positions.append(self.src.pos)
        return out


class Encryptor:
    """rgsw.NewEncryptor(params, sk): sk = (Q, P), NTT and Montgomery (P None without special primes)"""

    def __init__(self, oQ, oP, src: R.Source, sk, sigma=3.2, bound=19.2, exp=math.exp, log=R._log):
        self.oQ, self.oP, self.src, self.sk = oQ, oP, src, sk
        self.enc = _RlweEncryptor(oQ, oP, src, 2 / 3, sigma, bound, exp, log)
        self.gaussians = []  # per ciphertext encrypted: [u][row] the Gaussian drawn (limbs of Q)

    @property
    def positions(self):
        """the position of the source after every draw made so far (the uniform c1, then the Gaussian e, row after row)"""
        return self.enc.positions

    def encrypt_zero(self, levelQ, levelP, pw2=0):
        """EncryptZero on an *rgsw.Ciphertext (:77-121)"""
        oQ = self.oQ
        rows = KR.gadget_rows(oQ.moduli, levelQ, levelP, pw2)  # :85-86, :92-93
        keys = [{"q": np.zeros((len(rows), 2, levelQ + 1, oQ.N), dtype=np.uint64), "p": np.zeros((len(rows), 2, levelP + 1, oQ.N), dtype=np.uint64),
                 "pw2": pw2, "nj": KR.base_two_sizes(oQ.moduli, levelQ, levelP, pw2) if pw2 else None} for _ in range(2)]
        es = [[], []]
        for r in range(len(rows)):
            for u in range(2):  # :103-106 (levelP = -1: the ring.Poly element, the same draws) / :110-113
                n0 = len(self.enc.drawn)
                ((c0Q, c0P), (c1Q, c1P)), = self.enc.encrypt_zero_sk([self.sk], levelQ, levelP, 1, 1)
                es[u].append(self.enc.drawn[n0])
                keys[u]["q"][r, 0], keys[u]["q"][r, 1] = c0Q, c1Q
                if levelP >= 0:
                    keys[u]["p"][r, 0], keys[u]["p"][r, 1] = c0P, c1P
        self.gaussians.append(es)
        return keys

    def encrypt(self, pt, pt_is_ntt, pt_is_montgomery, levelQ, levelP, pw2=0):
        """Encrypt (:25-73); pt None: the nil plaintext"""
        oQ = self.oQ
        keys = self.encrypt_zero(levelQ, levelP, pw2)  # :33
        if pt is not None:
            buff = np.asarray(pt, dtype=np.uint64)[:levelQ + 1]
            if not pt_is_ntt:  # :47-52
                buff = oQ.NTT(buff)
            if not pt_is_montgomery:  # :50 / :55-56
                buff = oQ.unop("MForm", buff)
            KR.add_poly_times_gadget_vector(oQ, self.oP, buff, [keys[0]["q"], keys[1]["q"]], levelQ, levelP, pw2)  # :62-66
        return keys

    def encrypt_table(self, pts, sel, levelQ, levelP, pw2=0):
        """n successive Encrypt calls on the one source; pts [m][limbs][N], NTT and Montgomery"""
        return [self.encrypt(None if s < 0 else pts[s], True, True, levelQ, levelP, pw2) for s in sel]


def centered_lwe_secret(ringLWE, skLWE):
    """keys.go:51-58: INTT and IMForm at level 0, then PolyToBigintCentered (ring/ring.go:469-509: x >= Q >> 1 is x - Q)"""
    r0 = O.Ring(ringLWE.N, ringLWE.moduli[:1], ringLWE.conjugate_invariant)
    w = r0.unop("IMForm", r0.INTT(np.asarray(skLWE, dtype=np.uint64)[:1]))[0]
    q0 = int(ringLWE.moduli[0])
    return [int(x) - q0 if int(x) >= q0 >> 1 else int(x) for x in w]


def monomial(oQ, i):
    """NewMonomialXi (ring/ring.go:374-396) at the ring's full level"""
    N = oQ.N
    p = np.zeros((len(oQ.moduli), N), dtype=np.uint64)
    i &= (N << 1) - 1
    if i >= N:
        i -= N << 1
    for k, q in enumerate(oQ.moduli):
        if i < 0:
            p[k, N + i] = int(q) - 1
        else:
            p[k, i] = 1
    return p


def galois_elements(N):
    """keys.go:94-99"""
    return [pow(GALOIS_GEN, i + 1, 2 * N) for i in range(WINDOW_SIZE)] + [2 * N - GALOIS_GEN]


def gen_evaluation_key_new(oQ, oP, sk, ringLWE, skLWE, levelQ, levelP, pw2, src, src_kgen=None, sigma=3.2, bound=19.2, exp=math.exp, log=R._log):
    """GenEvaluationKeyNew (keys.go:46-108).  src_kgen None: the generator sits on the encryptor's source and draws after it.
    Returns (RGSW ciphertexts, {Galois element: key}, Gaussians of the RGSW ciphertexts, Gaussians of the Galois keys)"""
    s = centered_lwe_secret(ringLWE, skLWE)
    enc = Encryptor(oQ, oP, src, sk, sigma, bound, exp, log)  # :60
    ptXi = {}
    brk = []
    for si in s:  # :68-90
        if si not in ptXi:
            ptXi[si] = oQ.NTT(monomial(oQ, si))  # :77-78, IsNTT = true, IsMontgomery = false
        brk.append(enc.encrypt(ptXi[si], True, False, levelQ, levelP, pw2))
    kg = KR.KeyGenerator(oQ, oP, src if src_kgen is None else src_kgen, 2 / 3, sigma, bound, exp, log)  # :92
    els = galois_elements(oQ.N)
    gks = kg.gen_galois_keys(els, sk, levelQ, levelP, pw2)  # :101-105
    return brk, dict(zip(els, gks)), enc.gaussians, kg.gaussians


def image(ct):
    """the two keys as he_evk_download gives them: [2][rows][2][nQk + nPk][N]"""
    return np.stack([KR.image(ct[0]), KR.image(ct[1])])
