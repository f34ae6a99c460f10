"""The restatement of the multiparty key-generation protocols (tests/multiparty_ref.py) held against what the protocols promise, the
cases of the GPU tests (tests/multiparty_cases.py) held against the exp / log condition they rest on, the evaluation-key share held
against the formula of the kernel evk_finish, and the header's symbols.  No GPU."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as graft
from lattigo_amd import _lib
from tests import keygen_ref as KR
from tests import multiparty_aliasing as A
from tests import multiparty_cases as M
from tests import multiparty_ref as MR
from tests import sampler_ref as R
from tests.encryptor_cases import centered
from tests.multiparty_cases import crt_centered

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hering_multiparty.h")
BOUND = math.floor(M.BOUND)  # |e| <= 19 for every coefficient of every Gaussian: sampler_gaussian.go rejects beyond the bound 19.2


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ---- what a collective key is -----------------------------------------------------------------------------------------------------------
def small_of_rows(c, key, skIn, skOut):
    """per row (i, j): IMForm(INTT(c0 + c1 skOut)) minus the gadget term of skIn, centred -- asserted to be ONE polynomial on every Q
    and P limb"""
    oQ, oP = M.rings(c)
    out = []
    skOutQ, skOutP = skOut
    rows = KR.gadget_rows(c.Q, c.levelQ, c.levelP, c.pw2)
    P = math.prod(c.P[:c.levelP + 1])
    alpha = max(c.levelP + 1, 1)
    for r, (i, j) in enumerate(rows):
        x = oQ.binop("MulCoeffsMontgomeryThenAdd", key["q"][r, 1], skOutQ[:c.levelQ + 1], key["q"][r, 0])
        for k in range(alpha):
            index = i * alpha + k
            if index > c.levelQ:
                break
            q = c.Q[index]
            f = P * (1 << (j * c.pw2)) % q
            x[index] = np.array([(int(w) - int(s) * f) % q for w, s in zip(x[index], skIn[index])], dtype=np.uint64)
        e = oQ.unop("IMForm", oQ.INTT(x))
        small = centered(e[0], c.Q[0])
        for limb in range(c.levelQ + 1):
            assert centered(e[limb], c.Q[limb]) == small, (r, "Q", limb)
        if c.levelP >= 0:
            y = oP.unop("IMForm", oP.INTT(oP.binop("MulCoeffsMontgomeryThenAdd", key["p"][r, 1], skOutP[:c.levelP + 1], key["p"][r, 0])))
            for limb in range(c.levelP + 1):
                assert centered(y[limb], c.P[limb]) == small, (r, "P", limb)
        out.append(small)
    return out


def assert_collective_key(c, key, skIn, skOut, gaussians):
    """a key aggregated from len(gaussians) shares decrypts, row by row, to the gadget term of skIn plus the sum of the Gaussians the
    parties' restatements recorded for the row -- so the bound, parties x 19, is derived from them and not picked.  skIn, skOut: the
    sums of the parties' operands"""
    for r, small in enumerate(small_of_rows(c, key, skIn, skOut)):
        per_party = [centered(g[r][0], c.Q[0]) for g in gaussians]
        assert all(max(abs(v) for v in p) <= BOUND and any(p) for p in per_party)
        assert small == [sum(vs) for vs in zip(*per_party)], r
        assert max(abs(v) for v in small) <= len(gaussians) * BOUND


def _sum_operands(c, operands):
    oQ, oP = M.rings(c)
    skIn, (oq, op) = operands[0]
    skIn, oq = np.array(skIn[:c.levelQ + 1]), np.array(oq[:c.levelQ + 1])
    op = np.array(op[:c.levelP + 1]) if c.levelP >= 0 else None
    for i, (o0, o1) in operands[1:]:
        skIn, oq = oQ.binop("Add", skIn, i[:c.levelQ + 1]), oQ.binop("Add", oq, o0[:c.levelQ + 1])
        if op is not None:
            op = oP.binop("Add", op, o1[:c.levelP + 1])
    return skIn, (oq, op)


def _aggregate(c, shares):
    oQ, oP = M.rings(c)
    pr = MR.EvaluationKeyGenProtocol(oQ, oP, None)
    agg = shares[0]
    for s in shares[1:]:
        agg = pr.aggregate_shares(agg, s)
    return pr.gen_evaluation_key(agg, M.want_crp(c)[0])


@pytest.mark.parametrize("c", M.EVK_CASES, ids=lambda c: c.id)
def test_collective_evaluation_key_of_three_parties(c):
    runs = [M.want_evk_share(c, t) for t in range(M.PARTIES)]
    key = _aggregate(c, [r[0] for r in runs])
    skIn, skOut = _sum_operands(c, [r[3] for r in runs])
    assert_collective_key(c, key, skIn, skOut, [r[1] for r in runs])
    assert all(r[2] > 0 for r in runs) and M.want_crp(c)[1] > 0
    # the shares cycle the parties' keys, so the collective key switches from the summed key to the summed key
    assert np.array_equal(skIn, M.summed_secret(c, M.PARTIES)[0][:c.levelQ + 1]) and np.array_equal(skOut[0], skIn)


@pytest.mark.parametrize("c", M.GALOIS_CASES, ids=lambda c: c.id)
def test_collective_galois_key_of_three_parties(c):
    for g in M.galois_elements(c):
        runs = [M.want_galois_share(c, t, g) for t in range(M.PARTIES)]
        agg, key = M.want_collective_galois(c, M.PARTIES, g)
        assert len(agg) == M.PARTIES
        skIn, skOut = _sum_operands(c, [r[3] for r in runs])
        assert_collective_key(c, key, skIn, skOut, [r[1] for r in runs])
        # skOut is the automorphism of the summed key by the inverse element: what rlwe.KeyGenerator.GenGaloisKey hands genEvaluationKey
        oQ, oP = M.rings(c)
        kg = KR.KeyGenerator(oQ, oP, R.seeded_source(1))
        kg.gen_galois_key(g, M.summed_secret(c, M.PARTIES), c.levelQ, c.levelP, c.pw2)
        assert np.array_equal(kg.operands[0][1][0], skOut[0]) and np.array_equal(kg.operands[0][0][:c.levelQ + 1], skIn)


@pytest.mark.parametrize("parties", M.PARTY_COUNTS)
def test_aggregation_of_one_two_and_three_parties(parties):
    c = M.AGG_CASE
    runs = [M.want_evk_share(c, t) for t in range(parties)]
    key = _aggregate(c, [r[0] for r in runs])
    skIn, skOut = _sum_operands(c, [r[3] for r in runs])
    assert_collective_key(c, key, skIn, skOut, [r[1] for r in runs])


# ---- the drawing orders ------------------------------------------------------------------------------------------------------------------
def test_a_crp_is_the_uniform_draws_of_gen_evaluation_key_without_its_gaussians():
    """sampleCRP reads row after row, i outer: with the Gaussians cut out of the stream of genEvaluationKey the words are its c1"""
    c = M.EVK_CASES[0]
    crp, pos = M.want_crp(c)
    per_row = 8 * ((((c.levelQ + 1) * c.N + 127) // 128 * 128) + (((c.levelP + 1) * c.N + 127) // 128 * 128))
    assert pos == c.rows * per_row
    oQ, oP = M.rings(c)
    again = R.seeded_source(M.crs_seed(c))
    for r in range(c.rows):
        assert np.array_equal(crp["q"][r], np.array(R.uniform_read(again, c.N, c.Q[:c.levelQ + 1]), dtype=np.uint64))
        assert np.array_equal(crp["p"][r], np.array(R.uniform_read(again, c.N, c.P[:c.levelP + 1]), dtype=np.uint64))


def test_the_rejecting_modulus_moves_the_rows_of_the_crp():
    c = M.K.C_REJECT
    per_row = 8 * ((((c.levelQ + 1) * c.N + 127) // 128 * 128) + (((c.levelP + 1) * c.N + 127) // 128 * 128))
    assert M.want_crp(c)[1] > c.rows * per_row


@pytest.mark.parametrize("c", [M.K.C_B16, M.K.C_B7, M.K.C_B16_NOP], ids=lambda c: c.id)
def test_a_share_draws_j_outer_and_i_inner(c):
    """the t-th Gaussian of the party's stream is that of the t-th row in the order j outer, i inner -- not in row order"""
    _, gaussians, pos, _ = M.want_evk_share(c, 0)
    rows = KR.gadget_rows(c.Q, c.levelQ, c.levelP, c.pw2)
    order = sorted(range(len(rows)), key=lambda r: (rows[r][1], rows[r][0]))
    assert order != list(range(len(rows)))
    src = R.seeded_source(M.party_seed(c, 0))
    for r in order:
        e = np.array(R.gaussian_read(src, c.N, c.Q[:c.levelQ + 1], M.SIGMA, M.BOUND, False), dtype=np.uint64)
        assert np.array_equal(e, gaussians[r]), r
    assert src.pos == pos


# ---- the share is evk_finish with c1 := crp ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", M.EVK_CASES, ids=lambda c: c.id)
def test_the_share_is_the_evk_finish_formula_on_the_crp(c):
    """c0 = CRed(MForm(NTT(e)) + q - MRed(c1, skOut)), then CRed(c0 + MRed(skIn, MForm(P 2^(j pw2)))) on the Q limbs of the row's own
    digit: the kernel's two steps, in its order and with the canonical NTT, on the recorded e and c1 = crp"""
    oQ, oP = M.rings(c)
    share, gaussians, _, (skIn, (skOutQ, skOutP)) = M.want_evk_share(c, 0)
    crp = M.want_crp(c)[0]
    q = np.zeros((c.rows, 2, c.levelQ + 1, c.N), dtype=np.uint64)
    p = np.zeros((c.rows, 2, c.levelP + 1, c.N), dtype=np.uint64)
    for r in range(c.rows):
        e = gaussians[r]
        q[r, 1] = crp["q"][r]
        q[r, 0] = oQ.binop("MulCoeffsMontgomeryThenSub", crp["q"][r], skOutQ[:c.levelQ + 1], oQ.unop("MForm", oQ.NTT(e)))
        if c.levelP >= 0:
            from oracle import circuits as OC
            ep = OC.ExtendBasisSmallNormAndCenter(oQ, oP, e, c.levelP)
            p[r, 0] = oP.binop("MulCoeffsMontgomeryThenSub", crp["p"][r], skOutP[:c.levelP + 1], oP.unop("MForm", oP.NTT(ep)))
    KR.add_poly_times_gadget_vector(oQ, oP, skIn, [q], c.levelQ, c.levelP, c.pw2)
    assert np.array_equal(q[:, 0], share["q"]) and np.array_equal(p[:, 0], share["p"])
    for limb, m in enumerate(c.Q[:c.levelQ + 1]):
        assert int(share["q"][:, limb].max()) < m  # canonical


# ---- the stream check the GPU tests rest on ----------------------------------------------------------------------------------------------
def _same(a, b):
    return M.same_share(a[0], b[0]) and a[2] == b[2] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("c", M.EVK_CASES, ids=lambda c: c.id)
def test_no_evaluation_key_share_depends_on_exp_or_log(c):
    for t in range(1 if c.logN > 8 else M.PARTIES):
        base = M.want_evk_share(c, t)
        for ulps in (4, -4):
            assert _same(base, M.run_evk_share(c, t, R.shifted(math.exp, ulps), R.shifted(R._log, ulps))), (t, ulps)


@pytest.mark.parametrize("c", M.GALOIS_CASES, ids=lambda c: c.id)
def test_no_galois_share_depends_on_exp_or_log(c):
    for g in M.galois_elements(c):
        for t in range(M.PARTIES):
            base = M.want_galois_share(c, t, g)
            for ulps in (4, -4):
                assert _same(base, M.run_galois_share(c, t, g, R.shifted(math.exp, ulps), R.shifted(R._log, ulps))), (g, t, ulps)


# ---- the relinearization key ---------------------------------------------------------------------------------------------------------------
def negacyclic(a, b):
    """a b in Z[X]/(X^N + 1)"""
    N = len(a)
    out = [0] * N
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                if i + j < N:
                    out[i + j] += x * y
                else:
                    out[i + j - N] -= x * y
    return out


def small_key(c, q, levelQ=0):
    """the small polynomial of a key held NTT and Montgomery (limb 0)"""
    oQ, _ = M.rings(c)
    return centered(oQ.unop("IMForm", oQ.INTT(np.asarray(q)[:1]))[0], c.Q[0])


@pytest.mark.parametrize("c", [k for k in M.RKG_CASES if k.logN <= 8], ids=lambda c: c.id)
def test_collective_relinearization_key_of_three_parties(c):
    """with S, U, E0, E1, E2 the sums of the parties' secret keys, ephemeral keys and Gaussians: round one aggregates to
    [-U a + S P w + E0, S a + E1], round two to S h0 + (U - S) h1 + E2, so the key decrypts under S to P S^2 w plus, exactly,
    S E0 + U E1 + E2 -- the same polynomial on every Q and P limb.  Its bound follows from the recorded values: |S|, |U| <= 3 (ternary
    keys), |E| <= 3 x 19, N terms per product: 2 N 3 (3 x 19) + 3 x 19"""
    oQ, oP = M.rings(c)
    n = M.PARTIES
    r = M.want_rkg(c, n)
    S = M.summed_secret(c, n)
    sq = oQ.binop("MulCoeffsMontgomery", S[0], S[0])
    smalls = small_of_rows(c, r["rlk"], sq, S)
    s, us = small_key(c, S[0]), [small_key(c, e[0]) for e in r["eph"]]
    u = [sum(v) for v in zip(*us)]
    assert all(set(x) <= {-1, 0, 1} for x in us) and max(map(abs, s)) <= n
    bound = 2 * c.N * n * (n * BOUND) + n * BOUND
    for row, small in enumerate(smalls):
        E = [[sum(v) for v in zip(*[centered(g[row][k][0], c.Q[0]) for g in gs])] for gs, k in ((r["g1"], 0), (r["g1"], 1), (r["g2"], 0))]
        want = [a + b + e2 for a, b, e2 in zip(negacyclic(s, E[0]), negacyclic(u, E[1]), E[2])]
        assert small == want, row
        assert max(map(abs, small)) <= bound
    # round one is canonical; the ephemeral key keeps its ternary words above the share's level
    for t in range(n):
        assert all(int(r["share1"][t]["q"][:, :, limb].max()) < m for limb, m in enumerate(c.Q[:c.levelQ + 1]))
        for limb in range(c.levelQ + 1, len(c.Q)):
            assert set(int(w) for w in r["eph"][t][0][limb]) <= {0, 1, c.Q[limb] - 1}


@pytest.mark.parametrize("c", M.RKG_CASES, ids=lambda c: c.id)
def test_no_relinearization_round_depends_on_exp_or_log(c):
    n = M.rkg_parties(c)
    base = M.want_rkg(c, n)
    for ulps in (4, -4):
        assert M.same_rkg(base, M.run_rkg(c, n, R.shifted(math.exp, ulps), R.shifted(R._log, ulps))), ulps


def test_round_one_draws_the_ephemeral_key_first_and_two_gaussians_per_row():
    c = M.K.C_B7
    r = M.want_rkg(c, M.PARTIES)
    rows = KR.gadget_rows(c.Q, c.levelQ, c.levelP, c.pw2)
    src = R.seeded_source(M.party_seed(c, 0, 200))
    u = np.array(R.ternary_read(src, c.N, c.Q, M.XS_P, False), dtype=np.uint64)
    assert small_key(c, r["eph"][0][0]) == centered(u[0], c.Q[0])
    read = lambda: np.array(R.gaussian_read(src, c.N, c.Q[:c.levelQ + 1], M.SIGMA, M.BOUND, False), dtype=np.uint64)
    for row in sorted(range(len(rows)), key=lambda x: (rows[x][1], rows[x][0])):  # j outer, i inner
        assert np.array_equal(read(), r["g1"][0][row][0]) and np.array_equal(read(), r["g1"][0][row][1]), row
    assert src.pos == r["pos1"][0]
    for row in range(len(rows)):  # round two: i outer, j inner, on the same source
        assert np.array_equal(read(), r["g2"][0][row][0]), row
    assert src.pos == r["pos2"][0]


def test_the_lazy_shares_hold_words_at_or_above_the_modulus():
    """what makes the GPU comparison tell the reference's lazy word sequence from a canonicalising one: for the seeds chosen, the
    round-two share and the key-switch share (NTT branch) of the logN 13 case hold words in [q, 2q)"""
    c = M.K.C_BIG
    mods = np.array(c.Q[:c.levelQ + 1], dtype=np.uint64)
    r2 = M.want_rkg(c, 1)["share2"][0]["q"]
    assert (r2 >= mods[None, None, :, None]).any() and (r2 < 2 * mods[None, None, :, None]).all()
    ks = M.want_cks(c, c.levelQ, True)[0][0]
    assert (ks >= mods[:, None]).any() and (ks < 2 * mods[:, None]).all()


# ---- the public key --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", M.PK_CASES, ids=lambda c: c.id)
def test_collective_public_key(c):
    """pk = (sum of the shares, crp) decrypts under the summed key to the sum of the recorded Gaussians, on every Q and P limb"""
    oQ, oP = M.rings(c)
    n = 1 if c.logN > 8 else M.PARTIES
    crp, crs_pos, shares, pos, gs, agg = M.want_pk(c, n)
    S = M.summed_secret(c, n)
    small = [sum(v) for v in zip(*[centered(g[0], c.Q[0]) for g in gs])]
    assert max(map(abs, small)) <= n * BOUND and any(small)
    e = oQ.unop("IMForm", oQ.INTT(oQ.binop("MulCoeffsMontgomeryThenAdd", crp[0], S[0], agg[-1][0])))
    for limb, m in enumerate(c.Q):
        assert centered(e[limb], m) == small, limb
    if oP is not None:
        y = oP.unop("IMForm", oP.INTT(oP.binop("MulCoeffsMontgomeryThenAdd", crp[1], S[1], agg[-1][1])))
        for limb, m in enumerate(c.P):
            assert centered(y[limb], m) == small, limb
    assert crs_pos > 0 and all(p > 0 for p in pos)
    for ulps in (4, -4):
        again = M.run_pk(c, n, R.shifted(math.exp, ulps), R.shifted(R._log, ulps))
        assert again[3] == pos and all(np.array_equal(a[0], b[0]) for a, b in zip(again[2], shares)), ulps


# ---- the key switch --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_ntt", [True, False], ids=["ntt", "coefficients"])
@pytest.mark.parametrize("c", M.CKS_CASES, ids=lambda c: c.id)
def test_collective_key_switch(c, is_ntt):
    """c0 + sum of the shares, c1 decrypts under the summed target key to Delta m plus the sum of the parties' noise; each noise is
    within the sampler's bound 6 sigma, sigma = sqrt(NoiseFreshSK^2 + noise.Sigma^2), so the sum is within 3 x floor(6 sigma)"""
    oQ, oP = M.rings(c)
    level = c.levelQ
    mods = c.Q[:level + 1]
    m, Delta, c0, c1 = M.cks_input(c, level, is_ntt)
    shares, pos, gs, agg = M.want_cks(c, level, is_ntt)
    sigma, bound = MR.cks_noise(M.NOISE_FRESH_SK, M.CKS_NOISE_SIGMA)
    out0 = oQ.binop("Add", c0, agg[-1])  # KeySwitch (:143): one Add
    target = M.cks_target(c, 0)[0][:level + 1]
    for t in range(1, M.PARTIES):
        target = oQ.binop("Add", target, M.cks_target(c, t)[0][:level + 1])
    a0, a1 = (out0, c1) if is_ntt else (oQ.NTT(out0), oQ.NTT(c1))
    pt = oQ.INTT(oQ.binop("MulCoeffsMontgomeryThenAdd", a1, target, oQ.unop("Reduce", a0)))
    got = crt_centered(pt, mods)
    noise = [g - Delta * w for g, w in zip(got, m)]
    assert max(map(abs, noise)) <= M.PARTIES * math.floor(bound) and any(noise)
    if is_ntt:
        assert noise == [sum(v) for v in zip(*[centered(g[0], mods[0]) for g in gs])]
    assert all(p > 0 for p in pos)
    for ulps in (4, -4):
        again = M.run_cks(c, level, is_ntt, R.shifted(math.exp, ulps), R.shifted(R._log, ulps))
        assert again[1] == pos and all(np.array_equal(a, b) for a, b in zip(again[0], shares)), ulps


# ---- the public-key switch -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_ntt", [True, False], ids=["ntt", "coefficients"])
@pytest.mark.parametrize("c", M.PCKS_CASES, ids=lambda c: c.id)
def test_collective_public_key_switch(c, is_ntt):
    """(c0 + sum of share0, sum of share1) decrypts under the target secret key to Delta m plus, per party, a fresh encryption noise
    and a smudging Gaussian.  With |e| <= 19, u and s' ternary, e_pk the target key's own Gaussian: under encryptZeroPk (special
    primes, levelP = 0) |u e_pk + e0 + e1 s'| <= 19 (2 N + 1) divided by p_0, plus the ModDown rounding (1 + N) / 2; under
    encryptZeroPkNoP 19 (2 N + 1) itself.  Three parties: 3 (fresh + floor(6 sigma))"""
    oQ, oP = M.rings(c)
    level = c.levelQ
    mods = c.Q[:level + 1]
    m, Delta, c0, c1 = M.cks_input(c, level, is_ntt)
    shares, pos_enc, pos_noise, agg = M.want_pcks(c, level, is_ntt)
    sk, _ = M.pcks_target(c)
    _, bound = MR.cks_noise(M.NOISE_FRESH_SK, M.CKS_NOISE_SIGMA)
    fresh = BOUND * (2 * c.N + 1)
    fresh = fresh // c.P[0] + 1 + (1 + c.N) // 2 + 1 if c.P else fresh
    out0, out1 = oQ.binop("Add", c0, agg[-1][0]), agg[-1][1]  # KeySwitch (:127-140)
    a0, a1 = (out0, out1) if is_ntt else (oQ.NTT(out0), oQ.NTT(out1))
    pt = oQ.INTT(oQ.binop("MulCoeffsMontgomeryThenAdd", a1, sk[0][:level + 1], oQ.unop("Reduce", a0)))
    noise = [g - Delta * w for g, w in zip(crt_centered(pt, mods), m)]
    assert max(map(abs, noise)) <= M.PARTIES * (fresh + math.floor(bound)) and any(noise)
    assert all(p > 0 for p in pos_enc + pos_noise)
    for ulps in (4, -4):
        again = M.run_pcks(c, level, is_ntt, R.shifted(math.exp, ulps), R.shifted(R._log, ulps))
        assert again[1] == pos_enc and again[2] == pos_noise, ulps
        assert all(np.array_equal(x, y) for a, b in zip(again[0], shares) for x, y in zip(a, b)), ulps


# ---- the header ---------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_exported_and_left_out_of_recordings(lib):
    mine = sorted(set(re.findall(r"\b(he_[a-z0-9_]+)\s*\(", _header())))
    assert len(mine) == 11 and all(s.startswith("he_mp_") for s in mine), mine
    assert all(s in _lib.declared_symbols() and hasattr(lib, s) for s in mine), mine
    tables = (_lib._TRACE_FNS, _lib._TRACE_FNS_RGSW, _lib._TRACE_FNS_BLINDROT, _lib._TRACE_FNS_BRIDGE, _lib._TRACE_FNS_BFV)
    for s in mine:
        assert not any(s in t for t in tables), s  # no replay numbers
        assert s not in _lib._TRACE_IGNORE, s      # an entry carries the bytes of a source into a key: it fails a recording
    names = [lib.he_prof_kernel_name(i).decode() for i in range(64)]
    i = names.index("rgsw_table_finish")  # appended: earlier tests index the table
    assert names[i + 1:i + 5] == ["gadget_aggregate", "rkg_round_one", "rkg_round_two", "rlk_finalize"]


def test_prototypes_live_in_the_new_header_only():
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h.endswith((".h", ".hpp")) and h != "hering_multiparty.h":
            src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
            src = re.sub(r"//[^\n]*", "", src)
            assert not re.search(r"\bint\s+he_mp_[a-z0-9_]*\s*\(", src), h
    assert '#include "hering_keygen.h"' in open(HEADER).read()


def test_aliasing_table_covers_the_header():
    """every entry of the header has a row whose parameters are the header's key and polynomial operands, in order; ALLOWED is what
    the rows' verdicts accept"""
    entries = {}
    for m in re.finditer(r"\bint\s+(he_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", _header(), flags=re.S):
        ops = [p.split()[-1] for p in m.group(2).split(",") if "he_handle" in p and p.split()[-1] not in ("kgen", "eval", "crs", "enc", "noise_prng")]
        entries[m.group(1)] = ops
    assert sorted(entries) == sorted(A.ROWS)
    for name, ops in entries.items():
        assert list(A.ROWS[name].params) == ops, (name, ops)
    import itertools
    pairs = [(n, a, b) for n, r in A.ROWS.items() for a, b in itertools.combinations(r.params, 2)]
    accepted = sorted(p for p in pairs if p[1] in A.KEYS[p[0]] and p[2] in A.KEYS[p[0]] and A.ROWS[p[0]].verdict(p[1], p[2]) == "accept")
    assert all(A.ROWS[n].verdict(a, b) == "reject" and (a in A.KEYS[n]) == (b in A.KEYS[n]) for n, a, b in A.REFUSED)
    assert accepted == sorted(A.ALLOWED)


def test_the_go_abi_check_reads_the_new_header():
    src = open(os.path.join(ROOT, "tools", "check_go_abi.py")).read()
    assert src.count('"hering_multiparty.h"') == 1
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_go_abi.py")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
