"""The cases the multiparty tests share: the shapes of tests/keygen_cases.py, per-party secret keys and seeds, and the
restatement's result for each (tests/multiparty_ref.py), computed once.  tests/test_multiparty_host.py runs every case with exp / log
moved 4 ulps up and down and asks for identical words and positions, so that no Gaussian draw a GPU test compares depends on the
device's exp / log; a case that fails that check gets another seed, never a looser comparison."""
from __future__ import annotations

import functools
import math

import numpy as np

from tests import keygen_cases as K
from tests import keygen_ref as KR
from tests import multiparty_ref as MR
from tests import sampler_ref as R

Case = K.Case
XS_P, SIGMA, BOUND = K.XS_P, K.SIGMA, K.BOUND
PARTIES = 3
# the partial digit, the dividing chain, a key below the top levels, pw2 = 16 and 7 with P, pw2 = 16 without P, the class-boundary
# chains, the rejecting modulus (for the CRS draws), and logN 13 for the two-pass transform
EVK_CASES = [K.C_3P2, K.C_4P2, K.C_LOW, K.C_B16, K.C_B7, K.C_B16_NOP, K.C_CLASS, K.C_REJECT, K.C_BIG]
GALOIS_CASES = [K.C_3P2, K.C_CI]
PARTY_COUNTS = [1, 2, 3]
AGG_CASE = K.C_B7  # aggregation and finalisation on 1, 2 and 3 parties: rows of unequal digits, with P

rings = K.rings
galois_elements = K.galois_elements


def crs_seed(c: Case):
    return c.seed + 7000


def party_seed(c: Case, party: int, what: int = 0):
    return c.seed + 8000 + 100 * party + what


@functools.lru_cache(maxsize=None)
def secret(c: Case, party: int):
    """party's secret key at the evaluator's top levels, from a source of its own (the density sampler walks bits: no exp / log)"""
    oQ, oP = rings(c)
    kg = KR.KeyGenerator(oQ, oP, R.seeded_source(c.seed + 9000 + party), XS_P, SIGMA, BOUND)
    return kg.gen_secret_key(len(c.Q) - 1, len(c.P) - 1)


def summed_secret(c: Case, parties: int):
    oQ, oP = rings(c)
    q, p = secret(c, 0)
    for t in range(1, parties):
        q = oQ.binop("Add", q, secret(c, t)[0])
        p = oP.binop("Add", p, secret(c, t)[1]) if p is not None else None
    return q, p


@functools.lru_cache(maxsize=None)
def want_crp(c: Case):
    """(crp, the position of the CRS afterwards)"""
    oQ, oP = rings(c)
    crs = R.seeded_source(crs_seed(c))
    return MR.sample_crp(oQ, oP, crs, c.levelQ, c.levelP, c.pw2), crs.pos


def run_evk_share(c: Case, party: int, exp=math.exp, log=R._log):
    """party's share of the key from its own secret key to the next party's (skIn != skOut, so that neither is read for the other):
    (share, the Gaussians by row, the position of the party's source afterwards, (skIn, skOut))"""
    oQ, oP = rings(c)
    src = R.seeded_source(party_seed(c, party))
    pr = MR.EvaluationKeyGenProtocol(oQ, oP, src, SIGMA, BOUND, exp, log)
    share = pr.gen_share(secret(c, party)[0], secret(c, (party + 1) % PARTIES), want_crp(c)[0], c.levelQ, c.levelP, c.pw2)
    return share, pr.gaussians[0], src.pos, pr.operands[0]


def run_galois_share(c: Case, party: int, galEl: int, exp=math.exp, log=R._log):
    oQ, oP = rings(c)
    src = R.seeded_source(party_seed(c, party, 1 + galEl % 89))
    pr = MR.GaloisKeyGenProtocol(oQ, oP, src, SIGMA, BOUND, exp, log)
    share = pr.gen_share(secret(c, party), galEl, want_crp(c)[0], c.levelQ, c.levelP, c.pw2)
    return share, pr.gaussians[0], src.pos, pr.operands[0]


want_evk_share = functools.lru_cache(maxsize=None)(lambda c, party: run_evk_share(c, party))
want_galois_share = functools.lru_cache(maxsize=None)(lambda c, party, galEl: run_galois_share(c, party, galEl))


@functools.lru_cache(maxsize=None)
def want_collective_galois(c: Case, parties: int, galEl: int):
    """(the aggregated share after each party, the finalised key)"""
    oQ, oP = rings(c)
    pr = MR.GaloisKeyGenProtocol(oQ, oP, None)
    agg = [want_galois_share(c, 0, galEl)[0]]
    for t in range(1, parties):
        agg.append(pr.aggregate_shares(agg[-1], want_galois_share(c, t, galEl)[0]))
    nj = KR.base_two_sizes(c.Q, c.levelQ, c.levelP, c.pw2) if c.pw2 else None
    return agg, pr.gen_evaluation_key(agg[-1], want_crp(c)[0], c.pw2, nj)


def crt_centered(words, moduli):
    """[limbs][N] canonical words -> the centred integers modulo the product of the moduli"""
    Mq = math.prod(moduli)
    out = []
    for j in range(words.shape[1]):
        x = 0
        for i, q in enumerate(moduli):
            Mi = Mq // q
            x += int(words[i][j]) * Mi * pow(Mi, -1, q)
        x %= Mq
        out.append(x - Mq if x > Mq // 2 else x)
    return out


def same_share(a, b):
    return np.array_equal(a["q"], b["q"]) and np.array_equal(a["p"], b["p"])


# ---- the relinearization key ----------------------------------------------------------------------------------------------------------------
RKG_CASES = EVK_CASES


def rkg_parties(c: Case):
    return 1 if c.logN > 8 else PARTIES


def run_rkg(c: Case, parties: int, exp=math.exp, log=R._log):
    """the whole protocol among `parties`, each with ONE source for both rounds: dict of per-party lists eph, share1, pos1, share2, pos2,
    g1, g2 (the Gaussians by row), and agg1, agg2 (the aggregates after each party), rlk"""
    oQ, oP = rings(c)
    crp = want_crp(c)[0]
    out = {k: [] for k in ("eph", "share1", "pos1", "share2", "pos2", "g1", "g2", "agg1", "agg2")}
    prs = []
    for t in range(parties):
        src = R.seeded_source(party_seed(c, t, 200))
        pr = MR.RelinearizationKeyGenProtocol(oQ, oP, src, XS_P, SIGMA, BOUND, exp, log)
        prs.append(pr)
        eph, s1 = pr.gen_share_round_one(secret(c, t), crp, c.levelQ, c.levelP, c.pw2)
        out["eph"].append(eph), out["share1"].append(s1), out["pos1"].append(src.pos), out["g1"].append(pr.gaussians[0])
        out["agg1"].append(s1 if t == 0 else pr.aggregate_shares(out["agg1"][-1], s1))
    for t, pr in enumerate(prs):
        s2 = pr.gen_share_round_two(out["eph"][t], secret(c, t), out["agg1"][-1], c.levelQ, c.levelP, c.pw2)
        out["share2"].append(s2), out["pos2"].append(pr.src.pos), out["g2"].append(pr.gaussians[1])
        out["agg2"].append(s2 if t == 0 else pr.aggregate_shares(out["agg2"][-1], s2))
    nj = KR.base_two_sizes(c.Q, c.levelQ, c.levelP, c.pw2) if c.pw2 else None
    out["rlk"] = prs[0].gen_relinearization_key(out["agg1"][-1], out["agg2"][-1], c.pw2, nj)
    return out


want_rkg = functools.lru_cache(maxsize=None)(lambda c, parties: run_rkg(c, parties))


def same_rkg(a, b):
    return (a["pos1"] == b["pos1"] and a["pos2"] == b["pos2"] and all(same_share(x, y) for k in ("share1", "share2") for x, y in zip(a[k], b[k]))
            and all(np.array_equal(x[0], y[0]) for x, y in zip(a["eph"], b["eph"])) and KR.image(a["rlk"]).tobytes() == KR.image(b["rlk"]).tobytes())


# ---- the public key and the key switch -------------------------------------------------------------------------------------------------------
PK_CASES = [K.C_3P2, K.C_B16_NOP, K.C_CLASS, K.C_REJECT, K.C_BIG]  # with and without P; the rejecting modulus for the CRS; two passes
CKS_CASES = [K.C_3P2, K.C_CLASS, K.C_BIG]
NOISE_FRESH_SK, CKS_NOISE_SIGMA = SIGMA, 8 * SIGMA  # NoiseFreshSK is the parameters' Xe.Sigma; a flooding sigma of the tests' choosing


def run_pk(c: Case, parties: int, exp=math.exp, log=R._log):
    """(crp, the position of the CRS, shares, positions, Gaussians, the aggregates after each party)"""
    oQ, oP = rings(c)
    crs = R.seeded_source(crs_seed(c) + 1)
    crp = MR.PublicKeyGenProtocol(oQ, oP, None).sample_crp(crs)
    shares, pos, gs, agg = [], [], [], []
    for t in range(parties):
        src = R.seeded_source(party_seed(c, t, 300))
        pr = MR.PublicKeyGenProtocol(oQ, oP, src, SIGMA, BOUND, exp, log)
        shares.append(pr.gen_share(secret(c, t), crp))
        pos.append(src.pos), gs.append(pr.gaussians[0])
        agg.append(shares[-1] if t == 0 else pr.aggregate_shares(agg[-1], shares[-1]))
    return crp, crs.pos, shares, pos, gs, agg


def cks_input(c: Case, level: int, is_ntt: bool):
    """a ciphertext of Delta m under the summed key: (m, Delta, c0, c1) with c1 uniform and c0 = Delta m - c1 s exactly (no noise)"""
    oQ, _ = rings(c)
    rng = np.random.default_rng([c.seed, level, int(is_ntt)])
    mods = c.Q[:level + 1]
    m = [int(x) for x in rng.integers(0, 1 << 8, c.N)]
    Delta = math.prod(mods) >> 24
    c1 = np.stack([rng.integers(0, q, c.N, dtype=np.uint64) for q in mods])
    dm = oQ.NTT(np.stack([np.array([Delta * x % q for x in m], dtype=np.uint64) for q in mods]))
    s = summed_secret(c, PARTIES)[0][:level + 1]
    c0 = oQ.binop("Sub", dm, oQ.binop("MulCoeffsMontgomery", c1, s))
    if not is_ntt:
        c0, c1 = oQ.INTT(c0), oQ.INTT(c1)
    return m, Delta, c0, c1


@functools.lru_cache(maxsize=None)
def cks_target(c: Case, party: int):
    """party's share of the key the ciphertext is switched to"""
    oQ, oP = rings(c)
    return KR.KeyGenerator(oQ, oP, R.seeded_source(c.seed + 9500 + party), XS_P, SIGMA, BOUND).gen_secret_key(len(c.Q) - 1, len(c.P) - 1)


def run_cks(c: Case, level: int, is_ntt: bool, exp=math.exp, log=R._log):
    """(shares, positions, the NTT-branch Gaussians, the aggregates after each party)"""
    oQ, _ = rings(c)
    sigma, bound = MR.cks_noise(NOISE_FRESH_SK, CKS_NOISE_SIGMA)
    _, _, _, c1 = cks_input(c, level, is_ntt)
    shares, pos, gs, agg = [], [], [], []
    for t in range(PARTIES):
        src = R.seeded_source(party_seed(c, t, 400 + 2 * level + int(is_ntt)))
        pr = MR.KeySwitchProtocol(oQ, src, sigma, bound, exp, log)
        shares.append(pr.gen_share(secret(c, t)[0], cks_target(c, t)[0], c1, level, is_ntt))
        pos.append(src.pos), gs.append(pr.gaussians[0])
        agg.append(shares[-1] if t == 0 else oQ.binop("Add", agg[-1], shares[-1]))
    return shares, pos, gs, agg


want_pk = functools.lru_cache(maxsize=None)(lambda c, parties: run_pk(c, parties))
want_cks = functools.lru_cache(maxsize=None)(lambda c, level, is_ntt: run_cks(c, level, is_ntt))


# ---- the public-key switch ---------------------------------------------------------------------------------------------------------------------
PCKS_CASES = [K.C_3P2, K.C_B16_NOP]  # encryptZeroPk and encryptZeroPkNoP


@functools.lru_cache(maxsize=None)
def pcks_target(c: Case):
    """(sk, pk) the ciphertext is switched to: a key pair of one party's making, pk = (share, crp) of a one-party public-key protocol"""
    oQ, oP = rings(c)
    sk = cks_target(c, 0)
    pr = MR.PublicKeyGenProtocol(oQ, oP, R.seeded_source(c.seed + 9600), SIGMA, BOUND)
    crp = pr.sample_crp(R.seeded_source(c.seed + 9601))
    share = pr.gen_share(sk, crp)
    return sk, ((share[0], share[1]), (crp[0], crp[1]))


def run_pcks(c: Case, level: int, is_ntt: bool, exp=math.exp, log=R._log):
    """(shares, the positions of the encryptors' sources, the positions of the noise sources, the aggregates after each party)"""
    oQ, oP = rings(c)
    sigma, bound = MR.cks_noise(NOISE_FRESH_SK, CKS_NOISE_SIGMA)
    _, _, _, c1 = cks_input(c, level, is_ntt)
    _, pk = pcks_target(c)
    shares, pos_enc, pos_noise, agg = [], [], [], []
    for t in range(PARTIES):
        es, ns = R.seeded_source(party_seed(c, t, 500 + int(is_ntt))), R.seeded_source(party_seed(c, t, 510 + int(is_ntt)))
        pr = MR.PublicKeySwitchProtocol(oQ, oP, es, ns, sigma, bound, XS_P, SIGMA, BOUND, exp, log)
        shares.append(pr.gen_share(secret(c, t), pk, c1, level, is_ntt, False))
        pos_enc.append(es.pos), pos_noise.append(ns.pos)
        agg.append(shares[-1] if t == 0 else tuple(oQ.binop("Add", a, b) for a, b in zip(agg[-1], shares[-1])))
    return shares, pos_enc, pos_noise, agg


want_pcks = functools.lru_cache(maxsize=None)(lambda c, level, is_ntt: run_pcks(c, level, is_ntt))
