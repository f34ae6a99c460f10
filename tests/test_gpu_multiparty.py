"""The multiparty protocols on the device (include/hering_multiparty.h) against the restatement of the reference
(tests/multiparty_ref.py over the oracle's ring operations): every word, and the position of every source afterwards.  The cases are
those of tests/multiparty_cases.py, each of which has passed the host check that exp / log cannot change a word of it."""
import ctypes as C
import gc
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd import HeringError, sampling, wire
from lattigo_amd import encryptor as E
from lattigo_amd import keygen as G
from lattigo_amd import multiparty as MP
from tests import keygen_cases as K
from tests import keygen_ref as KR
from tests import multiparty_aliasing as A
from tests import multiparty_cases as M
from tests import multiparty_ref as MR
from tests import sampler_ref as R
from tests.gpu_common import ctx  # noqa: F401
from tests.multiparty_cases import crt_centered
from tests.test_gpu_keygen import Rig, negacyclic_auto, up

pytestmark = pytest.mark.gpu
HE_EINVAL, HE_EPRNG = -1, -6
_RIGS = {}


@pytest.fixture(scope="module", autouse=True)
def release_rigs():
    yield
    _RIGS.clear()
    gc.collect()


def rig(ctx, c) -> Rig:
    key = (c.logN, c.Q, c.P, c.ci)
    if key not in _RIGS:
        _RIGS[key] = Rig(ctx, c)
    return _RIGS[key]


def device_secret(rg, c, party):
    q, p = M.secret(c, party)
    return E.SecretKey(up(rg.gQ, q), up(rg.gP, p))


def party(rg, seed, cls=MP.EvaluationKeyGenProtocol):
    prng = sampling.PRNG(R.seeded_source(seed).read)
    return cls(G.KeyGenerator(rg.ev, prng, M.XS_P, M.SIGMA, M.BOUND)), prng


def params(c):
    return G.EvaluationKeyParameters(c.levelQ, c.levelP, c.pw2)


def key_of(rg, c, comp0=None, comp1=None):
    """a key handle of the case's shape with the given dicts (q, p by row) in its components, zeros elsewhere"""
    q = np.zeros((c.rows, 2, c.levelQ + 1, c.N), dtype=np.uint64)
    p = np.zeros((c.rows, 2, c.levelP + 1, c.N), dtype=np.uint64)
    for k, d in enumerate((comp0, comp1)):
        if d is not None:
            q[:, k], p[:, k] = d["q"], d["p"]
    nj = KR.base_two_sizes(c.Q, c.levelQ, c.levelP, c.pw2) if c.pw2 else None
    return rg.ev.NewEvaluationKey(q, p if c.levelP >= 0 else None, c.pw2, nj)


def device_crp(rg, c, cls=MP.EvaluationKeyGenCRP):
    return cls(key_of(rg, c, None, M.want_crp(c)[0]))


# ---- 1. word for word, position for position ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", M.EVK_CASES, ids=lambda c: c.id)
def test_sample_crp(ctx, c):
    rg = rig(ctx, c)
    want, pos = M.want_crp(c)
    pr, _ = party(rg, 1)
    crs = sampling.PRNG(R.seeded_source(M.crs_seed(c)).read)
    crp = pr.SampleCRP(crs, params(c))
    img = crp.key.download()
    assert img.shape == (c.rows, 2, c.levelQ + c.levelP + 2, c.N)
    assert np.array_equal(img[:, 1], MR.share_image(want)) and not img[:, 0].any()
    assert crs.Position() == pos


@pytest.mark.parametrize("c", M.EVK_CASES, ids=lambda c: c.id)
def test_evaluation_key_share(ctx, c):
    rg = rig(ctx, c)
    crp = device_crp(rg, c)
    for t in range(1 if c.logN > 8 else M.PARTIES):
        want, _, pos, _ = M.want_evk_share(c, t)
        pr, prng = party(rg, M.party_seed(c, t))
        share = pr.AllocateShare(params(c))
        pr.GenShare(device_secret(rg, c, t), device_secret(rg, c, (t + 1) % M.PARTIES), crp, share)
        img = share.key.download()
        assert np.array_equal(img[:, 0], MR.share_image(want)), t
        assert not img[:, 1].any()  # the other component stays
        assert prng.Position() == pos, t
    assert np.array_equal(crp.download(), MR.share_image(M.want_crp(c)[0]))


@pytest.mark.parametrize("c", M.GALOIS_CASES, ids=lambda c: c.id)
def test_galois_share(ctx, c):
    rg = rig(ctx, c)
    crp = device_crp(rg, c, MP.GaloisKeyGenCRP)
    for g in M.galois_elements(c):
        for t in range(M.PARTIES):
            want, _, pos, _ = M.want_galois_share(c, t, g)
            pr, prng = party(rg, M.party_seed(c, t, 1 + g % 89), MP.GaloisKeyGenProtocol)
            share = pr.AllocateShare(params(c))
            pr.GenShare(device_secret(rg, c, t), g, crp, share)
            assert share.GaloisElement == g
            assert np.array_equal(share.download(), MR.share_image(want)), (g, t)
            assert prng.Position() == pos, (g, t)


# ---- 2. aggregation and finalisation on 1, 2 and 3 parties -----------------------------------------------------------------------------
@pytest.mark.parametrize("parties", M.PARTY_COUNTS)
def test_collective_galois_key(ctx, parties):
    c, g = K.C_3P2, 5
    rg = rig(ctx, c)
    want_agg, want_key = M.want_collective_galois(c, parties, g)
    pr, _ = party(rg, 1, MP.GaloisKeyGenProtocol)
    crp = device_crp(rg, c, MP.GaloisKeyGenCRP)
    shares = [MP.GaloisKeyGenShare(key_of(rg, c, M.want_galois_share(c, t, g)[0]), g) for t in range(parties)]
    agg = shares[0]
    for t in range(1, parties):
        out = pr.AllocateShare(params(c))
        pr.AggregateShares(agg, shares[t], out)
        assert np.array_equal(out.download(), MR.share_image(want_agg[t])) and out.GaloisElement == g
        agg = out
    gk = G.GaloisKey(pr.kgen.NewEvaluationKey(params(c)), 0, 0)
    pr.GenGaloisKey(agg, crp, gk)
    assert (gk.GaloisElement, gk.NthRoot) == (g, rg.oQ.NthRoot())
    assert np.array_equal(gk.EvaluationKey.download(), KR.image(want_key))
    other = MP.GaloisKeyGenShare(shares[0].key, 7)
    with pytest.raises(ValueError):
        pr.AggregateShares(shares[0], other, shares[0])


@pytest.mark.parametrize("parties", M.PARTY_COUNTS)
def test_collective_evaluation_key_with_windows(ctx, parties):
    """pw2 = 7 with P: rows of two digits of unequal window counts"""
    c = M.AGG_CASE
    rg = rig(ctx, c)
    oQ, oP = M.rings(c)
    ref = MR.EvaluationKeyGenProtocol(oQ, oP, None)
    pr, _ = party(rg, 1)
    crp = device_crp(rg, c)
    want = M.want_evk_share(c, 0)[0]
    agg = MP.EvaluationKeyGenShare(key_of(rg, c, want))
    for t in range(1, parties):
        s = M.want_evk_share(c, t)[0]
        want = ref.aggregate_shares(want, s)
        pr.AggregateShares(agg, MP.EvaluationKeyGenShare(key_of(rg, c, s)), agg)  # in place
    evk = pr.kgen.NewEvaluationKey(params(c))
    pr.GenEvaluationKey(agg, crp, evk)
    assert np.array_equal(evk.download(), KR.image(ref.gen_evaluation_key(want, M.want_crp(c)[0])))


@pytest.mark.parametrize("degree", [0, 1])
@pytest.mark.parametrize("c", [K.C_3P2, K.C_B16_NOP, K.C_CLASS], ids=lambda c: c.id)
def test_aggregate_is_one_conditional_subtraction(ctx, c, degree):
    """words anywhere in [0, 2q), as the lazy shares of the relinearization protocol hold them: out = a + b, minus q once when the sum
    reaches q (ring.Add) -- words in [q, 3q) included, which a full reduction would change; components above `degree` stay"""
    rg = rig(ctx, c)
    rng = np.random.default_rng([c.seed, degree])
    mods = list(c.Q[:c.levelQ + 1]) + list(c.P[:c.levelP + 1])

    def words():
        return np.stack([[[rng.integers(0, 2 * m, c.N, dtype=np.uint64) for m in mods] for _ in range(2)] for _ in range(c.rows)])

    def key(img):
        nj = KR.base_two_sizes(c.Q, c.levelQ, c.levelP, c.pw2) if c.pw2 else None
        return rg.ev.NewEvaluationKey(img[:, :, :c.levelQ + 1], img[:, :, c.levelQ + 1:] if c.levelP >= 0 else None, c.pw2, nj)

    a, b, o = words(), words(), words()
    a[0, 0, 0, :4] = [0, mods[0] - 1, 2 * mods[0] - 1, 1]
    b[0, 0, 0, :4] = [0, 1, 2 * mods[0] - 1, mods[0] - 1]
    want = o.copy()
    mq = np.array(mods, dtype=np.uint64)[None, None, :, None]
    s = a + b
    want[:, :degree + 1] = np.where(s >= mq, s - mq, s)[:, :degree + 1]
    assert (want[:, :degree + 1] >= mq).any()  # the comparison tells one CRed from a canonicalising sum
    ka, kb, ko = key(a), key(b), key(o)
    la.load().he_mp_gadget_aggregate.restype = C.c_int
    assert la.load().he_mp_gadget_aggregate(ka.h, kb.h, degree, ko.h) == 0
    assert np.array_equal(ko.download(), want)
    assert np.array_equal(ka.download(), a) and np.array_equal(kb.download(), b)


# ---- 3. the aliasing rows ---------------------------------------------------------------------------------------------------------------
def test_operands_that_may_be_one_handle(ctx):
    c = K.C_B16
    rg = rig(ctx, c)
    L = la.load()
    crpw = M.want_crp(c)[0]
    pairs = set()
    # crp and share one handle: the handle then holds the key
    want, _, pos, _ = M.want_evk_share(c, 0)
    pr, prng = party(rg, M.party_seed(c, 0))
    both = device_crp(rg, c)
    pr.GenShare(device_secret(rg, c, 0), device_secret(rg, c, 1), both, MP.EvaluationKeyGenShare(both.key))
    img = both.key.download()
    assert np.array_equal(img[:, 0], MR.share_image(want)) and np.array_equal(img[:, 1], MR.share_image(crpw)) and prng.Position() == pos
    pairs |= {("he_mp_evk_gen_share", "crp", "share")}
    g = 5
    wantg, _, posg, _ = M.want_galois_share(c, 0, g)
    prg, prngg = party(rg, M.party_seed(c, 0, 1 + g % 89), MP.GaloisKeyGenProtocol)
    bothg = device_crp(rg, c, MP.GaloisKeyGenCRP)
    prg.GenShare(device_secret(rg, c, 0), g, bothg, MP.GaloisKeyGenShare(bothg.key))
    assert np.array_equal(bothg.key.download()[:, 0], MR.share_image(wantg)) and prngg.Position() == posg
    pairs |= {("he_mp_galois_gen_share", "crp", "share")}
    # finalize on the handle that holds both: nothing moves
    evk = both.key
    assert L.he_mp_evk_finalize(evk.h, evk.h, evk.h) == 0 and np.array_equal(evk.download(), img)
    pairs |= {("he_mp_evk_finalize", "share", "crp"), ("he_mp_evk_finalize", "share", "evk"), ("he_mp_evk_finalize", "crp", "evk")}
    # skIn and skOut.Q one polynomial (the Q and P parts of a key are read only: nothing to tell apart)
    sk0 = device_secret(rg, c, 0)
    oQ, oP = M.rings(c)
    ref = MR.EvaluationKeyGenProtocol(oQ, oP, R.seeded_source(77), M.SIGMA, M.BOUND)
    wself = ref.gen_share(M.secret(c, 0)[0], M.secret(c, 0), crpw, c.levelQ, c.levelP, c.pw2)
    pr2, _ = party(rg, 77)
    sh = pr2.AllocateShare(params(c))
    pr2.GenShare(sk0, sk0, device_crp(rg, c), sh)
    assert np.array_equal(sh.download(), MR.share_image(wself))
    # aggregate: a + a, into a, into b
    a, b = key_of(rg, c, want), key_of(rg, c, wself)
    s_ab, s_aa = ref.aggregate_shares(want, wself), ref.aggregate_shares(want, want)
    out = key_of(rg, c)
    assert L.he_mp_gadget_aggregate(a.h, a.h, 0, out.h) == 0 and np.array_equal(out.download()[:, 0], MR.share_image(s_aa))
    assert L.he_mp_gadget_aggregate(a.h, b.h, 0, b.h) == 0 and np.array_equal(b.download()[:, 0], MR.share_image(s_ab))
    b = key_of(rg, c, wself)
    assert L.he_mp_gadget_aggregate(a.h, b.h, 0, a.h) == 0 and np.array_equal(a.download()[:, 0], MR.share_image(s_ab))
    pairs |= {("he_mp_gadget_aggregate", "a", "b"), ("he_mp_gadget_aggregate", "a", "out"), ("he_mp_gadget_aggregate", "b", "out")}
    # GenRelinearizationKey into round2, and with one handle for both rounds
    rng = np.random.default_rng(3)
    mods = list(c.Q[:c.levelQ + 1]) + list(c.P[:c.levelP + 1])
    words = lambda: {"q": np.stack([[rng.integers(0, m, c.N, dtype=np.uint64) for m in c.Q[:c.levelQ + 1]] for _ in range(c.rows)]),
                     "p": np.stack([[rng.integers(0, m, c.N, dtype=np.uint64) for m in c.P[:c.levelP + 1]] for _ in range(c.rows)])}
    w = [words() for _ in range(4)]
    mf = lambda d: np.concatenate([np.stack([oQ.unop("MForm", x) for x in d["q"]]), np.stack([oP.unop("MForm", x) for x in d["p"]])], axis=1)
    r1, r2 = key_of(rg, c, w[0], w[1]), key_of(rg, c, w[2], w[3])
    assert L.he_mp_rlk_finalize(r1.h, r2.h, r2.h) == 0
    assert np.array_equal(r2.download(), np.stack([mf(w[2]), mf(w[1])], axis=1))
    assert L.he_mp_rlk_finalize(r1.h, r1.h, r1.h) == 0
    assert np.array_equal(r1.download(), np.stack([mf(w[0]), mf(w[1])], axis=1))
    pairs |= {("he_mp_rlk_finalize", "round1", "round2"), ("he_mp_rlk_finalize", "round1", "rlk"), ("he_mp_rlk_finalize", "round2", "rlk")}
    assert pairs == set(A.ALLOWED) and len(mods) == c.levelQ + c.levelP + 2


# ---- 4. a collective key behaves as the same words uploaded ---------------------------------------------------------------------------------
def test_finalized_key_behaves_as_uploaded(ctx):
    """on the class chain, whose limb below 2^47 gives the key its derived double-precision copy: finalisation must refresh it"""
    c = K.C_CLASS
    rg = rig(ctx, c)
    pr, _ = party(rg, M.party_seed(c, 0))
    crs = sampling.PRNG(R.seeded_source(M.crs_seed(c)).read)
    crp = pr.SampleCRP(crs, params(c))
    share = MP.EvaluationKeyGenShare(crp.key)
    pr.GenShare(device_secret(rg, c, 0), device_secret(rg, c, 1), crp, share)
    evk = crp.key
    pr.GenEvaluationKey(share, crp, evk)
    img = evk.download()
    assert np.array_equal(img[:, 0], MR.share_image(M.want_evk_share(c, 0)[0]))
    again = rg.ev.NewEvaluationKey(img[:, :, :c.levelQ + 1], img[:, :, c.levelQ + 1:])
    cx = up(rg.gQ, K.uniform_poly(c, 6))
    outs = []
    for key in (evk, again):
        ct = [rg.gQ.NewPoly(), rg.gQ.NewPoly()]
        rg.ev.GadgetProduct(c.levelQ, cx, key, ct)
        outs.append([x.download() for x in ct])
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and outs[0][0].any()


# ---- 5. end to end: three parties on the device, every intermediate against the restatement ------------------------------------------------------
def test_three_parties_end_to_end(ctx):
    """logN 6, three parties, each with ONE seeded source for everything it draws (and one for its smudging noise in the public-key
    switch), the restatement (tests/multiparty_ref.py, tests/keygen_ref.py, tests/encryptor_ref.py and the oracle's Evaluator) run on
    the same sources in the same order: the secret keys; the collective public key, relinearization key and Galois key (every CRP,
    share, aggregate and finalised key); Encrypt under the collective public key; the tensor square of that ciphertext Relinearized;
    Automorphism; the collective key switch to three fresh keys and the collective public-key switch to a fresh key pair; Decrypt.
    EVERY intermediate is compared word for word and every source position checked; the decryptions return the message.

    The decryptions' bounds, N = 64, Q of 4 limbs, P of 2 limbs, beta = 2, |e| <= 19 per Gaussian, so |S| <= 3 and |E| <= 57:
      fresh under the collective pk (levelP = 0, ModDown by p_0): F = (N 57 + 19 + N 19 3) / p_0 + (1 + 3 N) / 2;
      a key switch under a collective key whose rows carry noise within K: beta N K max(D_i) / P + (1 + 3 N) / 2, with K = 57 for the
          Galois key and K = 2 N 3 57 + 57 for the relinearization key (tests/test_multiparty_host.py);
      the square: |(Delta m + e)^2 - Delta^2 m^2| <= N (2 Delta 2^16 F + F^2), plus the relinearization's;
      the key switches add three Gaussians within floor(6 sigma) each, sigma = sqrt(3.2^2 + 25.6^2); the public-key switch also three
          fresh encryptions under a one-party key: 3 ((19 (2 N + 1)) / p_0 + (1 + N) / 2)."""
    from tests import encryptor_ref as ER
    from oracle import oracle as O
    c = K.C_4P2
    rg = rig(ctx, c)
    N, Q, P, n = c.N, c.Q, c.P, 3
    oQ, oP = rg.oQ, rg.oP
    lq, lp = len(Q) - 1, len(P) - 1
    alpha, beta = len(P), KR.base_rns_size(lq, lp)
    Dmax = max(math.prod(Q[i * alpha:(i + 1) * alpha]) for i in range(beta))
    Delta = 1 << 40
    F = Fraction(N * 57 + 19 + N * 19 * 3, P[0]) + Fraction(1 + 3 * N, 2)
    ks = lambda Kn: Fraction(beta * N * Kn * Dmax, math.prod(P)) + Fraction(1 + 3 * N, 2)
    sigma, bound = MR.cks_noise(M.NOISE_FRESH_SK, M.CKS_NOISE_SIGMA)
    B_auto, B_sq = F + ks(57), N * (2 * Delta * (1 << 16) * F + F * F) + ks(2 * N * 3 * 57 + 57)
    B_cks, B_pcks = F + 3 * math.floor(bound), F + 3 * math.floor(bound) + 3 * (Fraction(19 * (2 * N + 1), P[0]) + Fraction(1 + N, 2))
    assert 4 * max(F, B_auto, B_cks, B_pcks) <= Delta and 4 * B_sq <= Delta * Delta and Delta * Delta * (1 << 32) * N * 4 < math.prod(Q)

    seeds = [7100 + t for t in range(n)]
    srcs, nsrcs = [R.seeded_source(s) for s in seeds], [R.seeded_source(s + 50) for s in seeds]
    prngs, nprngs = [sampling.PRNG(R.seeded_source(s).read) for s in seeds], [sampling.PRNG(R.seeded_source(s + 50).read) for s in seeds]
    crs_ref, crs = R.seeded_source(7200), sampling.PRNG(R.seeded_source(7200).read)
    kgs = [G.KeyGenerator(rg.ev, g, M.XS_P, M.SIGMA, M.BOUND) for g in prngs]
    rkgs = [KR.KeyGenerator(oQ, oP, s, M.XS_P, M.SIGMA, M.BOUND) for s in srcs]
    img = lambda pol: pol.download()[0]
    qp = lambda x: (img(x.Q), img(x.P))
    eq = lambda got, want: all(np.array_equal(g, w) for g, w in zip(got, want))

    def positions(what):
        assert [g.Position() for g in prngs] == [s.pos for s in srcs], what
        assert [g.Position() for g in nprngs] == [s.pos for s in nsrcs] and crs.Position() == crs_ref.pos, what

    def summed(keys):
        q, p = keys[0]
        for k in keys[1:]:
            q, p = oQ.binop("Add", q, k[0]), oP.binop("Add", p, k[1])
        return q, p

    # -- secret keys, and the fresh keys of the key switch
    sks, wsk = [kg.GenSecretKeyNew() for kg in kgs], [r.gen_secret_key(lq, lp) for r in rkgs]
    tgs, wtg = [kg.GenSecretKeyNew() for kg in kgs], [r.gen_secret_key(lq, lp) for r in rkgs]
    assert all(eq(qp(a), b) for a, b in zip(sks + tgs, wsk + wtg))
    positions("secret keys")
    wS, wT = summed(wsk), summed(wtg)
    sk_sum, tg_sum = E.SecretKey(up(rg.gQ, wS[0]), up(rg.gP, wS[1])), E.SecretKey(up(rg.gQ, wT[0]), up(rg.gP, wT[1]))

    # -- the collective public key
    pks, rpks = [MP.PublicKeyGenProtocol(kg) for kg in kgs], [MR.PublicKeyGenProtocol(oQ, oP, s, M.SIGMA, M.BOUND) for s in srcs]
    pcrp, wpcrp = pks[0].SampleCRP(crs), rpks[0].sample_crp(crs_ref)
    assert eq(qp(pcrp), wpcrp)
    pagg = wpagg = None
    for t in range(n):
        share, wshare = pks[t].AllocateShare(), rpks[t].gen_share(wsk[t], wpcrp)
        pks[t].GenShare(sks[t], pcrp, share)
        assert eq(qp(share), wshare), t
        if pagg is None:
            pagg, wpagg = share, wshare
        else:
            pks[t].AggregateShares(pagg, share, pagg)
            wpagg = rpks[t].aggregate_shares(wpagg, wshare)
            assert eq(qp(pagg), wpagg), t
    pk = E.PublicKey(((rg.gQ.NewPoly(), rg.gP.NewPoly()), (rg.gQ.NewPoly(), rg.gP.NewPoly())))
    pks[0].GenPublicKey(pagg, pcrp, pk)
    wpk = (wpagg, wpcrp)
    assert all(eq((img(v[0]), img(v[1])), w) for v, w in zip(pk.Value, wpk))
    positions("public key")

    # -- the collective relinearization key
    rks, rrks = [MP.RelinearizationKeyGenProtocol(kg) for kg in kgs], [MR.RelinearizationKeyGenProtocol(oQ, oP, s, M.XS_P, M.SIGMA, M.BOUND) for s in srcs]
    rcrp, wrcrp = rks[0].SampleCRP(crs), MR.sample_crp(oQ, oP, crs_ref, lq, lp)
    assert np.array_equal(rcrp.download(), MR.share_image(wrcrp))
    alloc, weph, agg1, wagg1 = [pr.AllocateShare() for pr in rks], [], None, None
    for t in range(n):
        eph, r1, _ = alloc[t]
        rks[t].GenShareRoundOne(sks[t], rcrp, eph, r1)
        we, w1 = rrks[t].gen_share_round_one(wsk[t], wrcrp, lq, lp)
        weph.append(we)
        assert np.array_equal(r1.download(), MR.gadget_image(w1)) and eq(qp(eph), we), t
        if agg1 is None:
            agg1, wagg1 = r1, w1
        else:
            rks[t].AggregateShares(agg1, r1, agg1)
            wagg1 = rrks[t].aggregate_shares(wagg1, w1)
            assert np.array_equal(agg1.download(), MR.gadget_image(wagg1)), t
    positions("round one")
    agg2 = wagg2 = None
    for t in range(n):
        eph, _, r2 = alloc[t]
        rks[t].GenShareRoundTwo(eph, sks[t], agg1, r2)
        w2 = rrks[t].gen_share_round_two(weph[t], wsk[t], wagg1, lq, lp)
        assert np.array_equal(r2.download(), MR.gadget_image(w2)), t
        if agg2 is None:
            agg2, wagg2 = r2, w2
        else:
            rks[t].AggregateShares(agg2, r2, agg2)
            wagg2 = rrks[t].aggregate_shares(wagg2, w2)
            assert np.array_equal(agg2.download(), MR.gadget_image(wagg2)), t
    rlk = kgs[0].NewEvaluationKey()
    rks[0].GenRelinearizationKey(agg1, agg2, rlk)
    wrlk = rrks[0].gen_relinearization_key(wagg1, wagg2)
    assert np.array_equal(rlk.download(), KR.image(wrlk))
    positions("relinearization key")

    # -- the collective Galois key of 5
    g = 5
    gps, rgps = [MP.GaloisKeyGenProtocol(kg) for kg in kgs], [MR.GaloisKeyGenProtocol(oQ, oP, s, M.SIGMA, M.BOUND) for s in srcs]
    gcrp, wgcrp = gps[0].SampleCRP(crs), MR.sample_crp(oQ, oP, crs_ref, lq, lp)
    assert np.array_equal(gcrp.download(), MR.share_image(wgcrp))
    gagg = wgagg = None
    for t in range(n):
        share, wshare = gps[t].AllocateShare(), rgps[t].gen_share(wsk[t], g, wgcrp, lq, lp)
        gps[t].GenShare(sks[t], g, gcrp, share)
        assert np.array_equal(share.download(), MR.share_image(wshare)), t
        if gagg is None:
            gagg, wgagg = share, wshare
        else:
            gps[t].AggregateShares(gagg, share, gagg)
            wgagg = rgps[t].aggregate_shares(wgagg, wshare)
            assert np.array_equal(gagg.download(), MR.share_image(wgagg)), t
    gk = G.GaloisKey(kgs[0].NewEvaluationKey(), 0, 0)
    gps[0].GenGaloisKey(gagg, gcrp, gk)
    wgk = rgps[0].gen_evaluation_key(wgagg, wgcrp)
    assert np.array_equal(gk.EvaluationKey.download(), KR.image(wgk)) and (gk.GaloisElement, gk.NthRoot) == (g, oQ.NthRoot())
    positions("Galois key")

    # -- Encrypt under the collective public key (party 0's encryptor, on its own source)
    rng = np.random.default_rng(23)
    m = [int(x) for x in rng.integers(0, 1 << 16, N)]
    dm = oQ.NTT(np.stack([np.array([Delta * x % q for x in m], dtype=np.uint64) for q in Q]))
    ct = E.Element([rg.gQ.NewPoly(), rg.gQ.NewPoly()])
    E.Encryptor(rg.ev, prngs[0], pk, M.XS_P, M.SIGMA, M.BOUND).Encrypt(E.Plaintext(up(rg.gQ, dm), True, False), ct)
    renc = ER.Encryptor(oQ, oP, srcs[0], M.XS_P, M.SIGMA, M.BOUND)
    ((w0, _), (w1, _)), = renc.encrypt_zero_pk([wpk], lq, 0, False, True, False)
    wct = np.stack([renc.add_pt_to_ct(lq, dm, True, w0, True), w1])
    assert eq([img(v) for v in ct.Value], wct)
    positions("encrypt")

    def decrypts_to(polys, key, want, scale, B, what):
        pt = E.Plaintext(rg.gQ.NewPoly())
        E.Decryptor(rg.ev, key).Decrypt(E.Element(polys, True, False), pt)
        got = crt_centered(oQ.INTT(img(pt.Value)), Q)
        noise = max(abs(x - scale * w) for x, w in zip(got, want))
        print(what, "noise", float(noise), "bound", float(B))
        assert [(x + scale // 2) // scale for x in got] == want and noise <= B, what

    decrypts_to(ct.Value, sk_sum, m, Delta, F, "fresh under the collective public key")

    # -- the tensor square (on the oracle: no new code), Relinearize under the collective key
    oev = O.Evaluator(oQ, oP)
    bar = lambda a, b: oQ.binop("MulCoeffsBarrett", a, b)
    d1 = bar(wct[0], wct[1])
    wd = np.stack([bar(wct[0], wct[0]), oQ.binop("Add", d1, d1), bar(wct[1], wct[1])])
    out = [rg.gQ.NewPoly(), rg.gQ.NewPoly()]
    rg.ev.Relinearize(lq, [up(rg.gQ, x) for x in wd], rlk, out)
    assert eq([img(v) for v in out], oev.Relinearize(wd, O.EvaluationKey(wrlk["q"], wrlk["p"])))
    mm = [0] * N
    for i, a in enumerate(m):
        for j, b in enumerate(m):
            k = i + j
            mm[k % N] += a * b if k < N else -a * b
    decrypts_to(out, sk_sum, mm, Delta * Delta, B_sq, "square, relinearized")

    # -- Automorphism under the collective Galois key
    out = [rg.gQ.NewPoly(), rg.gQ.NewPoly()]
    rg.ev.Automorphism(lq, ct.Value, g, gk.EvaluationKey, out)
    assert eq([img(v) for v in out], oev.Automorphism(wct, g, O.EvaluationKey(wgk["q"], wgk["p"])))
    decrypts_to(out, sk_sum, negacyclic_auto(m, g), Delta, B_auto, "automorphism")

    # -- the collective key switch to the fresh keys
    kss = [MP.KeySwitchProtocol(kg, M.CKS_NOISE_SIGMA, M.NOISE_FRESH_SK) for kg in kgs]
    rkss = [MR.KeySwitchProtocol(oQ, s, sigma, bound) for s in srcs]
    kagg = wkagg = None
    for t in range(n):
        share, wshare = kss[t].AllocateShare(lq), rkss[t].gen_share(wsk[t][0], wtg[t][0], wct[1], lq, True)
        kss[t].GenShare(sks[t], tgs[t], ct, share)
        assert np.array_equal(img(share.Value), wshare), t
        if kagg is None:
            kagg, wkagg = share, wshare
        else:
            kss[t].AggregateShares(kagg, share, kagg)
            wkagg = oQ.binop("Add", wkagg, wshare)
            assert np.array_equal(img(kagg.Value), wkagg), t
    sw = E.Element([rg.gQ.NewPoly(), rg.gQ.NewPoly()])
    kss[0].KeySwitch(ct, kagg, sw)
    wsw = np.stack([oQ.binop("Add", wct[0], wkagg), wct[1]])
    assert eq([img(v) for v in sw.Value], wsw)
    positions("key switch")
    decrypts_to([up(rg.gQ, oQ.unop("Reduce", wsw[0])), sw.Value[1]], tg_sum, m, Delta, B_cks, "collective key switch")

    # -- the collective public-key switch to a fresh key pair (made by a fourth generator)
    src4, prng4 = R.seeded_source(7400), sampling.PRNG(R.seeded_source(7400).read)
    kg4, rkg4 = G.KeyGenerator(rg.ev, prng4, M.XS_P, M.SIGMA, M.BOUND), KR.KeyGenerator(oQ, oP, src4, M.XS_P, M.SIGMA, M.BOUND)
    sk4, pk4 = kg4.GenKeyPairNew()
    wsk4 = rkg4.gen_secret_key(lq, lp)
    wpk4, = rkg4.enc.encrypt_zero_sk([wsk4], lq, lp, 1, 1)
    assert eq(qp(sk4), wsk4) and all(eq((img(v[0]), img(v[1])), w) for v, w in zip(pk4.Value, wpk4)) and prng4.Position() == src4.pos
    pcs = [MP.PublicKeySwitchProtocol(E.Encryptor(rg.ev, prngs[t], None, M.XS_P, M.SIGMA, M.BOUND), nprngs[t], M.CKS_NOISE_SIGMA, M.NOISE_FRESH_SK)
           for t in range(n)]
    rpcs = [MR.PublicKeySwitchProtocol(oQ, oP, srcs[t], nsrcs[t], sigma, bound, M.XS_P, M.SIGMA, M.BOUND) for t in range(n)]
    cagg = wcagg = None
    for t in range(n):
        share, wshare = pcs[t].AllocateShare(lq), rpcs[t].gen_share(wsk[t], wpk4, wct[1], lq, True, False)
        pcs[t].GenShare(sks[t], pk4, ct, share)
        assert eq([img(v) for v in share.Value], wshare), t
        if cagg is None:
            cagg, wcagg = share, wshare
        else:
            pcs[t].AggregateShares(cagg, share, cagg)
            wcagg = tuple(oQ.binop("Add", a, b) for a, b in zip(wcagg, wshare))
            assert eq([img(v) for v in cagg.Value], wcagg), t
    sw = E.Element([rg.gQ.NewPoly(), rg.gQ.NewPoly()])
    pcs[0].KeySwitch(ct, cagg, sw)
    wsw = np.stack([oQ.binop("Add", wct[0], wcagg[0]), wcagg[1]])
    assert eq([img(v) for v in sw.Value], wsw)
    positions("public-key switch")
    assert all(s.pos > 0 for s in srcs + nsrcs)
    decrypts_to([up(rg.gQ, oQ.unop("Reduce", wsw[0])), up(rg.gQ, oQ.unop("Reduce", wsw[1]))], sk4, m, Delta, B_pcks, "collective public-key switch")


# ---- 6. the wire form ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [K.C_3P2, K.C_B7, K.C_B16_NOP], ids=lambda c: c.id)
def test_wire_form_of_shares_and_crps(ctx, c):
    rg = rig(ctx, c)
    want = M.want_evk_share(c, 0)[0]
    nj = KR.base_two_sizes(c.Q, c.levelQ, c.levelP, c.pw2) if c.pw2 else [1] * c.rows
    size = 16 + sum(8 + n * (8 + wire.poly_binary_size(c.levelQ + 1, c.N) + wire.poly_binary_size(c.levelP + 1, c.N)) for n in nj)  # gadgetciphertext.go:86
    for obj, words, lead in ((MP.EvaluationKeyGenShare(key_of(rg, c, want)), want, b""),
                             (MP.GaloisKeyGenShare(key_of(rg, c, want), 5), want, struct.pack("<Q", 5)),
                             (device_crp(rg, c), M.want_crp(c)[0], b"")):
        buf = obj.MarshalBinary()
        assert len(buf) == obj.BinarySize() == size + len(lead) and buf[:len(lead)] == lead
        q, p, pw2, nj2 = wire.gadget_ciphertext_unmarshal(buf[len(lead):])
        assert q.shape[1] == 1 and pw2 == c.pw2 and nj2 == nj
        assert np.array_equal(q[:, 0], words["q"]) and np.array_equal(p[:, 0].reshape(words["p"].shape), words["p"])
    # RelinearizationKeyGenShare: 2 components for round one, 1 for round two
    r = M.want_rkg(c, 1)
    for w, degree in ((r["share1"][0], 1), (r["share2"][0], 0)):
        obj = MP.RelinearizationKeyGenShare(key_of(rg, c, halves(w, 0), halves(w, 1) if degree else None), degree)
        per = 8 + (degree + 1) * (wire.poly_binary_size(c.levelQ + 1, c.N) + wire.poly_binary_size(c.levelP + 1, c.N))
        buf = obj.MarshalBinary()
        assert len(buf) == obj.BinarySize() == 16 + sum(8 + k * per for k in nj)
        q, p, pw2, nj2 = wire.gadget_ciphertext_unmarshal(buf)
        assert q.shape[1] == degree + 1 and pw2 == c.pw2 and nj2 == nj
        assert np.array_equal(q, w["q"]) and np.array_equal(p.reshape(w["p"].shape), w["p"])


# ---- 7. launches --------------------------------------------------------------------------------------------------------------------------
def census(ctx, c, call):
    call()  # (once outside: the scratch has its size)
    ctx.sync()
    ctx.prof_begin()
    call()
    ctx.sync()
    prof = ctx.prof_end()
    return sum(v[0] for v in prof.values()), prof


def test_launch_census(ctx):
    """he_mp_evk_gen_share: one launch per row (its Gaussian) and, whatever the number of rows, 4 after the last draw (3 without
    special primes): the two expansions, one transform, one evk_finish.  he_mp_gadget_aggregate: one launch; he_mp_crp_gadget: one
    per row"""
    after = {}
    for c in (K.C_4P2, K.C_LOW, K.C_B7, K.C_B16_NOP):
        rg = rig(ctx, c)
        pr, _ = party(rg, 3)
        crp = device_crp(rg, c)
        share = pr.AllocateShare(params(c))
        sk0, sk1 = device_secret(rg, c, 0), device_secret(rg, c, 1)
        n, prof = census(ctx, c, lambda: pr.GenShare(sk0, sk1, crp, share))
        print(c.id, "rows", c.rows, "launches", n, {k: v[0] for k, v in prof.items()})
        assert prof["evk_finish"][0] == 1 and prof["sampler_gaussian"][0] == c.rows and "sampler_uniform" not in {k for k, v in prof.items() if v[0]}
        assert n == c.rows + (4 if c.levelP >= 0 else 3)
        after[c.id] = n - c.rows
        n, prof = census(ctx, c, lambda: pr.AggregateShares(share, share, share))
        assert n == 1 and prof["gadget_aggregate"][0] == 1
        crs = sampling.PRNG(R.seeded_source(9).read)
        n, prof = census(ctx, c, lambda: la.load().he_mp_crp_gadget(rg.ev.h, crs.h, crp.key.h))
        assert n == c.rows and prof["sampler_uniform"][0] == c.rows
    print(after)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------
def refused(call, code=HE_EINVAL):
    with pytest.raises(HeringError) as e:
        call()
    assert e.value.code == code, e.value


def test_refusals_touch_nothing(ctx):
    c = K.C_3P2
    rg = rig(ctx, c)
    sk = device_secret(rg, c, 0)
    pr, prng = party(rg, 1, MP.GaloisKeyGenProtocol)
    crp = device_crp(rg, c, MP.GaloisKeyGenCRP)
    good = pr.AllocateShare()
    low = pr.AllocateShare(G.EvaluationKeyParameters(1, 1, 0))            # a share at other levels than the crp
    odd = MP.GaloisKeyGenShare(la.EvaluationKey(rg.ev, None, None, shape=(3, 3, 2)))  # beta against the levels
    other = Rig(ctx, c)
    foreign = MP.GaloisKeyGenShare(la.EvaluationKey(other.ev, None, None, shape=(2, 3, 2)))  # a key of another evaluator
    evk = MP.EvaluationKeyGenProtocol(pr.kgen)
    for bad in (low, odd, foreign):
        refused(lambda: pr.GenShare(sk, 5, crp, bad))
        refused(lambda: evk.GenShare(sk, sk, crp, bad))
        refused(lambda: evk.AggregateShares(good, bad, good))
        refused(lambda: evk.AggregateShares(bad, good, good))
        refused(lambda: evk.AggregateShares(good, good, bad))
        refused(lambda: evk.GenEvaluationKey(bad, crp, good.key))
        refused(lambda: evk.GenEvaluationKey(good, crp, bad.key))
    crs = sampling.PRNG(R.seeded_source(2).read)
    refused(lambda: crs.check(la.load().he_mp_crp_gadget(other.ev.h, crs.h, good.key.h)))
    refused(lambda: crs.check(la.load().he_mp_crp_gadget(rg.ev.h, crs.h, odd.key.h)))
    refused(lambda: la._lib.check(la.load().he_mp_gadget_aggregate(good.key.h, good.key.h, 2, good.key.h)))
    refused(lambda: la._lib.check(la.load().he_mp_gadget_aggregate(good.key.h, good.key.h, -1, good.key.h)))
    sk3 = E.SecretKey(rg.gQ.NewPoly(3), rg.gP.NewPoly(3))
    refused(lambda: pr.GenShare(sk3, 5, crp, good))     # a batch-3 secret key
    refused(lambda: evk.GenShare(sk, sk3, crp, good))
    refused(lambda: pr.GenShare(sk, 4, crp, good))      # an even Galois element
    assert prng.Position() == 0 and crs.Position() == 0 and not good.key.download().any()
    assert np.array_equal(crp.download(), MR.share_image(M.want_crp(c)[0]))
    # a conjugate-invariant ring has the automorphisms 5^k alone
    cc = K.C_CI
    ci = rig(ctx, cc)
    prci, prngci = party(ci, 2, MP.GaloisKeyGenProtocol)
    refused(lambda: prci.GenShare(device_secret(ci, cc, 0), ci.oQ.NthRoot() - 1, device_crp(ci, cc, MP.GaloisKeyGenCRP), prci.AllocateShare(params(cc))))
    assert prngci.Position() == 0


def test_refused_inside_a_graph_capture(ctx):
    c = K.C_3P2
    rg = rig(ctx, c)
    sk = device_secret(rg, c, 0)
    pr, prng = party(rg, 3, MP.GaloisKeyGenProtocol)
    evk = MP.EvaluationKeyGenProtocol(pr.kgen)
    crp = device_crp(rg, c, MP.GaloisKeyGenCRP)
    share = pr.AllocateShare()
    evk.GenShare(sk, sk, crp, share)  # (once outside, as a capture asks)
    crs = sampling.PRNG(R.seeded_source(4).read)
    pos, img = prng.Position(), share.key.download()
    L = la.load()
    codes = []
    gc.collect()  # (a key of an earlier test released by the collector during the capture would synchronise the stream)
    assert L.he_graph_begin(ctx.h) == 0
    try:
        codes = [L.he_mp_evk_gen_share(pr.kgen.h, sk.Q.h, sk.Q.h, sk.P.h, crp.key.h, share.key.h),
                 L.he_mp_galois_gen_share(pr.kgen.h, 5, sk.Q.h, sk.P.h, crp.key.h, share.key.h),
                 L.he_mp_gadget_aggregate(share.key.h, share.key.h, 0, share.key.h),
                 L.he_mp_evk_finalize(share.key.h, crp.key.h, share.key.h), L.he_mp_crp_gadget(rg.ev.h, crs.h, share.key.h)]
    finally:
        g = C.c_uint64()
        rc = L.he_graph_end(ctx.h, C.byref(g))
        assert rc == 0, L.he_last_error()
        L.he_graph_destroy(g.value)
    assert codes == [HE_EINVAL] * 5
    assert prng.Position() == pos and crs.Position() == 0 and np.array_equal(share.key.download(), img)


def test_a_failing_source_is_eprng_and_consumes_nothing(ctx):
    c = K.C_3P2
    rg = rig(ctx, c)
    sk = device_secret(rg, c, 0)
    prng = sampling.PRNG(lambda n: b"")  # a short read
    pr = MP.GaloisKeyGenProtocol(G.KeyGenerator(rg.ev, prng))
    evk = MP.EvaluationKeyGenProtocol(pr.kgen)
    crp = device_crp(rg, c, MP.GaloisKeyGenCRP)
    share = pr.AllocateShare()
    for call in (lambda: evk.GenShare(sk, sk, crp, share), lambda: pr.GenShare(sk, 5, crp, share), lambda: pr.SampleCRP(prng)):
        refused(call, HE_EPRNG)
        assert prng.Position() == 0


# ---- 9. the relinearization key ------------------------------------------------------------------------------------------------------------
def halves(share, k):
    """component k of a restated share as the dict key_of takes"""
    return {"q": share["q"][:, k], "p": share["p"][:, k]}


def rkg_party(rg, c, t):
    prng = sampling.PRNG(R.seeded_source(M.party_seed(c, t, 200)).read)
    return MP.RelinearizationKeyGenProtocol(G.KeyGenerator(rg.ev, prng, M.XS_P, M.SIGMA, M.BOUND)), prng


@pytest.mark.parametrize("c", M.RKG_CASES, ids=lambda c: c.id)
def test_relinearization_rounds(ctx, c):
    """both rounds of every party on ONE source per party, word for word: the ephemeral key (its ternary words above the share's level
    included), the canonical round-one share, the lazy round-two share, and the position after each round"""
    rg = rig(ctx, c)
    n = M.rkg_parties(c)
    want = M.want_rkg(c, n)
    crp = device_crp(rg, c, MP.RelinearizationKeyGenCRP)
    agg1 = MP.RelinearizationKeyGenShare(key_of(rg, c, halves(want["agg1"][-1], 0), halves(want["agg1"][-1], 1)), 1)
    mods = np.array(list(c.Q[:c.levelQ + 1]) + list(c.P[:c.levelP + 1]), dtype=np.uint64)[None, None, :, None]
    for t in range(n):
        pr, prng = rkg_party(rg, c, t)
        sk = device_secret(rg, c, t)
        eph, r1, r2 = pr.AllocateShare(params(c))
        pr.GenShareRoundOne(sk, crp, eph, r1)
        assert np.array_equal(r1.download(), MR.gadget_image(want["share1"][t])), t
        assert np.array_equal(eph.Q.download()[0], want["eph"][t][0]), t
        if c.levelP >= 0:
            assert np.array_equal(eph.P.download()[0][:c.levelP + 1], want["eph"][t][1]), t
        assert prng.Position() == want["pos1"][t], t
        pr.GenShareRoundTwo(eph, sk, agg1, r2)
        img = r2.key.download()
        assert np.array_equal(img[:, :1], MR.gadget_image(want["share2"][t])) and not img[:, 1].any(), t
        assert prng.Position() == want["pos2"][t], t
        if c is K.C_BIG:
            assert (img[:, :1] >= mods).any()  # the lazy word sequence, not a canonicalising one
    assert np.array_equal(agg1.download(), MR.gadget_image(want["agg1"][-1]))


@pytest.mark.parametrize("parties", M.PARTY_COUNTS)
@pytest.mark.parametrize("c", [K.C_3P2, K.C_B7], ids=lambda c: c.id)
def test_collective_relinearization_key(ctx, c, parties):
    rg = rig(ctx, c)
    want = M.want_rkg(c, parties)
    pr, _ = rkg_party(rg, c, 0)
    r1 = [MP.RelinearizationKeyGenShare(key_of(rg, c, halves(s, 0), halves(s, 1)), 1) for s in want["share1"]]
    r2 = [MP.RelinearizationKeyGenShare(key_of(rg, c, halves(s, 0)), 0) for s in want["share2"]]
    for t in range(1, parties):
        pr.AggregateShares(r1[0], r1[t], r1[0])
        pr.AggregateShares(r2[0], r2[t], r2[0])
        assert np.array_equal(r1[0].download(), MR.gadget_image(want["agg1"][t])) and np.array_equal(r2[0].download(), MR.gadget_image(want["agg2"][t]))
    rlk = pr.kgen.NewEvaluationKey(params(c))
    pr.GenRelinearizationKey(r1[0], r2[0], rlk)
    assert np.array_equal(rlk.download(), KR.image(want["rlk"]))
    pr.GenRelinearizationKey(r1[0], r2[0], r1[0].key)  # in place on round1
    assert np.array_equal(r1[0].key.download(), KR.image(want["rlk"]))


def test_rlk_finalize_is_mform_of_lazy_words(ctx):
    """MForm on words anywhere in [0, 2q) -- what an aggregated round-two share may hold -- against the oracle's MForm"""
    c = K.C_CLASS
    rg = rig(ctx, c)
    rng = np.random.default_rng(c.seed)
    mods = list(c.Q[:c.levelQ + 1]) + list(c.P[:c.levelP + 1])
    img = [np.stack([[[rng.integers(0, 2 * m, c.N, dtype=np.uint64) for m in mods] for _ in range(2)] for _ in range(c.rows)]) for _ in range(2)]
    keys = [rg.ev.NewEvaluationKey(x[:, :, :c.levelQ + 1], x[:, :, c.levelQ + 1:]) for x in img]
    out = rg.ev.NewEvaluationKey(img[0][:, :, :c.levelQ + 1], img[0][:, :, c.levelQ + 1:])
    assert la.load().he_mp_rlk_finalize(keys[0].h, keys[1].h, out.h) == 0
    want = np.stack([np.stack([np.concatenate([rg.oQ.unop("MForm", src[r, k, :c.levelQ + 1]), rg.oP.unop("MForm", src[r, k, c.levelQ + 1:])])
                               for k, src in ((0, img[1]), (1, img[0]))]) for r in range(c.rows)])
    assert np.array_equal(out.download(), want)


# ---- 10. the public key ----------------------------------------------------------------------------------------------------------------------
def qp_image(x):
    return x.Q.download()[0], (x.P.download()[0] if x.P is not None else None)


def same_qp(got, want):
    return np.array_equal(got[0], want[0]) and (want[1] is None or np.array_equal(got[1], want[1]))


@pytest.mark.parametrize("c", M.PK_CASES, ids=lambda c: c.id)
def test_collective_public_key(ctx, c):
    rg = rig(ctx, c)
    n = 1 if c.logN > 8 else M.PARTIES
    wcrp, crs_pos, shares, pos, _, agg = M.want_pk(c, n)
    crs = sampling.PRNG(R.seeded_source(M.crs_seed(c) + 1).read)
    agg_dev = None
    for t in range(n):
        prng = sampling.PRNG(R.seeded_source(M.party_seed(c, t, 300)).read)
        pr = MP.PublicKeyGenProtocol(G.KeyGenerator(rg.ev, prng, M.XS_P, M.SIGMA, M.BOUND))
        if t == 0:
            crp = pr.SampleCRP(crs)
            assert same_qp(qp_image(crp), wcrp) and crs.Position() == crs_pos
        share = pr.AllocateShare()
        pr.GenShare(device_secret(rg, c, t), crp, share)
        assert same_qp(qp_image(share), shares[t]) and prng.Position() == pos[t], t
        if agg_dev is None:
            agg_dev = share
        else:
            pr.AggregateShares(agg_dev, share, agg_dev)
            assert same_qp(qp_image(agg_dev), agg[t]), t
    new = lambda: (rg.gQ.NewPoly(), rg.gP.NewPoly() if rg.gP is not None else None)
    pk = E.PublicKey((new(), new()))
    pr.GenPublicKey(agg_dev, crp, pk)
    assert same_qp((pk.Value[0][0].download()[0], pk.Value[0][1].download()[0] if rg.gP is not None else None), agg[-1])
    assert same_qp((pk.Value[1][0].download()[0], pk.Value[1][1].download()[0] if rg.gP is not None else None), wcrp)
    buf, nq = agg_dev.MarshalBinary(), wire.poly_binary_size(len(c.Q), c.N)  # ringqp.Poly.WriteTo: Q, then P
    assert len(buf) == agg_dev.BinarySize() == nq + wire.poly_binary_size(len(c.P), c.N)
    assert np.array_equal(wire.poly_unmarshal(buf[:nq]), agg[-1][0])
    assert rg.gP is None or np.array_equal(wire.poly_unmarshal(buf[nq:]), agg[-1][1])


# ---- 11. the key switch ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_ntt", [True, False], ids=["ntt", "coefficients"])
@pytest.mark.parametrize("c", M.CKS_CASES, ids=lambda c: c.id)
def test_collective_key_switch(ctx, c, is_ntt):
    rg = rig(ctx, c)
    level = c.levelQ
    _, _, c0, c1 = M.cks_input(c, level, is_ntt)
    shares, pos, _, agg = M.want_cks(c, level, is_ntt)
    rq = rg.gQ.AtLevel(level)
    ct = E.Element([la.Poly(rq, level + 1, 1).upload(c0[None]), la.Poly(rq, level + 1, 1).upload(c1[None])], is_ntt, False)
    mods = np.array(c.Q[:level + 1], dtype=np.uint64)[:, None]
    agg_dev = None
    for t in range(M.PARTIES):
        prng = sampling.PRNG(R.seeded_source(M.party_seed(c, t, 400 + 2 * level + int(is_ntt))).read)
        pr = MP.KeySwitchProtocol(G.KeyGenerator(rg.ev, prng, M.XS_P, M.SIGMA, M.BOUND), M.CKS_NOISE_SIGMA, M.NOISE_FRESH_SK)
        assert (pr.Sigma, pr.Bound) == MR.cks_noise(M.NOISE_FRESH_SK, M.CKS_NOISE_SIGMA)
        share = pr.AllocateShare(level)
        tq, tp = M.cks_target(c, t)
        pr.GenShare(device_secret(rg, c, t), E.SecretKey(up(rg.gQ, tq), up(rg.gP, tp)), ct, share)
        got = share.Value.download()[0]
        assert np.array_equal(got, shares[t]) and prng.Position() == pos[t], t
        if c is K.C_BIG and is_ntt and t == 0:
            assert (got >= mods).any()  # the lazy words of :103, as the reference leaves them
        assert wire.poly_unmarshal(share.MarshalBinary()).tobytes() == shares[t].tobytes() and len(share.MarshalBinary()) == share.BinarySize()
        if agg_dev is None:
            agg_dev = share
        else:
            pr.AggregateShares(agg_dev, share, agg_dev)
            assert np.array_equal(agg_dev.Value.download()[0], agg[t]), t
    out = E.Element([rq.NewPoly(), rq.NewPoly()], not is_ntt, True)
    pr.KeySwitch(ct, agg_dev, out)
    assert np.array_equal(out.Value[0].download()[0], rg.oQ.binop("Add", c0, agg[-1])) and np.array_equal(out.Value[1].download()[0], c1)
    assert (out.IsNTT, out.IsMontgomery) == (is_ntt, False)
    assert np.array_equal(ct.Value[1].download()[0], c1)


# ---- 11b. the public-key switch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_ntt", [True, False], ids=["ntt", "coefficients"])
@pytest.mark.parametrize("c", M.PCKS_CASES, ids=lambda c: c.id)
def test_collective_public_key_switch(ctx, c, is_ntt):
    """both sources of every party, both branches, with encryptZeroPk and (no special primes) encryptZeroPkNoP"""
    rg = rig(ctx, c)
    level = c.levelQ
    _, _, c0, c1 = M.cks_input(c, level, is_ntt)
    shares, pos_enc, pos_noise, agg = M.want_pcks(c, level, is_ntt)
    _, wpk = M.pcks_target(c)
    pk = E.PublicKey(tuple((up(rg.gQ, q), up(rg.gP, p)) for q, p in wpk))
    ct = E.Element([up(rg.gQ, c0), up(rg.gQ, c1)], is_ntt, False)
    agg_dev = None
    for t in range(M.PARTIES):
        es = sampling.PRNG(R.seeded_source(M.party_seed(c, t, 500 + int(is_ntt))).read)
        ns = sampling.PRNG(R.seeded_source(M.party_seed(c, t, 510 + int(is_ntt))).read)
        pr = MP.PublicKeySwitchProtocol(E.Encryptor(rg.ev, es, None, M.XS_P, M.SIGMA, M.BOUND), ns, M.CKS_NOISE_SIGMA, M.NOISE_FRESH_SK)
        share = pr.AllocateShare(level)
        pr.GenShare(device_secret(rg, c, t), pk, ct, share)
        got = [v.download()[0] for v in share.Value]
        assert np.array_equal(got[0], shares[t][0]) and np.array_equal(got[1], shares[t][1]), t
        assert (es.Position(), ns.Position()) == (pos_enc[t], pos_noise[t]), t
        buf = share.MarshalBinary()  # Element.BinarySize (core/rlwe/element.go:315-322) with the MetaData of rlwe.NewElement
        assert len(buf) == share.BinarySize() == 1 + wire.METADATA_BINARY_SIZE + 8 + 2 * wire.poly_binary_size(level + 1, c.N)
        value, meta = wire.ciphertext_unmarshal(buf)
        assert np.array_equal(value, np.stack(shares[t])) and meta["is_ntt"] and not meta["is_montgomery"]
        if agg_dev is None:
            agg_dev = share
        else:
            pr.AggregateShares(agg_dev, share, agg_dev)
            assert all(np.array_equal(v.download()[0], w) for v, w in zip(agg_dev.Value, agg[t])), t
    out = E.Element([rg.gQ.NewPoly(), rg.gQ.NewPoly()], not is_ntt, True)
    pr.KeySwitch(ct, agg_dev, out)
    assert np.array_equal(out.Value[0].download()[0], rg.oQ.binop("Add", c0, agg[-1][0])) and np.array_equal(out.Value[1].download()[0], agg[-1][1])
    assert (out.IsNTT, out.IsMontgomery) == (is_ntt, False)
    # refusals: no public key bound; a share below the level; a share that is an input
    L = la.load()
    bare = E.Encryptor(rg.ev, es, None, M.XS_P, M.SIGMA, M.BOUND)
    sk, s0, s1 = device_secret(rg, c, 0), rg.gQ.NewPoly(), rg.gQ.NewPoly()
    enc = E.Encryptor(rg.ev, es, pk, M.XS_P, M.SIGMA, M.BOUND)
    pe, pn = es.Position(), ns.Position()
    call = lambda e, lvl, a, b: L.he_mp_pcks_gen_share(e.h, ns.h, lvl, sk.Q.h, ct.Value[1].h, 1, 0, 3.2, 19.2, a.h, b.h)
    assert call(bare, level, s0, s1) == HE_EINVAL
    assert call(enc, level, rg.gQ.AtLevel(level - 1).NewPoly(), s1) == HE_EINVAL
    assert call(enc, level + 1, s0, s1) == HE_EINVAL
    assert call(enc, level, s0, s0) == HE_EINVAL and call(enc, level, sk.Q, s1) == HE_EINVAL and call(enc, level, s0, ct.Value[1]) == HE_EINVAL
    assert (es.Position(), ns.Position()) == (pe, pn) and not s0.download().any() and not s1.download().any()
    dead = sampling.PRNG(lambda n: b"")
    assert L.he_mp_pcks_gen_share(enc.h, dead.h, level, sk.Q.h, ct.Value[1].h, 1, 0, 3.2, 19.2, s0.h, s1.h) == HE_EPRNG and dead.Position() == 0


# ---- 12. launches, refusals and failing sources of the later entries ---------------------------------------------------------------------------
def test_launch_census_of_the_relinearization_rounds(ctx):
    """one launch per row (its Gaussians: round one parses both of a row in one) and, whatever the number of rows, 4 after the last
    draw (3 without special primes): two expansions, ONE transform over all rows and components, ONE launch of the round's kernel"""
    extra = {}
    for c in (K.C_4P2, K.C_B7, K.C_B16_NOP):
        rg = rig(ctx, c)
        pr, _ = rkg_party(rg, c, 0)
        sk = device_secret(rg, c, 0)
        crp = device_crp(rg, c, MP.RelinearizationKeyGenCRP)
        eph, r1, r2 = pr.AllocateShare(params(c))
        tail = 4 if c.levelP >= 0 else 3
        n, prof = census(ctx, c, lambda: pr.GenShareRoundOne(sk, crp, eph, r1))
        print(c.id, "round one: rows", c.rows, "launches", n, {k: v[0] for k, v in prof.items() if v[0]})
        assert prof["rkg_round_one"][0] == 1 and prof["sampler_gaussian"][0] == c.rows
        extra[c.id] = n - c.rows - tail  # the ephemeral key
        agg1 = MP.RelinearizationKeyGenShare(key_of(rg, c, halves(M.want_rkg(c, 1)["share1"][0], 0), halves(M.want_rkg(c, 1)["share1"][0], 1)), 1)
        n, prof = census(ctx, c, lambda: pr.GenShareRoundTwo(eph, sk, agg1, r2))
        print(c.id, "round two: rows", c.rows, "launches", n, {k: v[0] for k, v in prof.items() if v[0]})
        assert prof["rkg_round_two"][0] == 1 and prof["sampler_gaussian"][0] == c.rows and n == c.rows + tail
        n, prof = census(ctx, c, lambda: pr.GenRelinearizationKey(agg1, r2, pr.kgen.NewEvaluationKey(params(c))))
        assert prof["rlk_finalize"][0] == 1
    print("launches of the ephemeral key", extra)
    assert extra == {K.C_4P2.id: 7, K.C_B7.id: 7, K.C_B16_NOP.id: 4}  # the same work whatever the rows


def test_launch_census_of_the_other_entries(ctx):
    """the counts the header states for the polynomial-sized shares, the finalisations and the two-pass transform"""
    L = la.load()
    total = lambda prof: sum(v[0] for v in prof.values())
    for c, want_pk in ((K.C_3P2, 9), (K.C_B16_NOP, 5)):  # he_mp_pk_gen_share: 9 with special primes, 5 without
        rg = rig(ctx, c)
        prng = sampling.PRNG(R.seeded_source(5).read)
        kg = G.KeyGenerator(rg.ev, prng, M.XS_P, M.SIGMA, M.BOUND)
        pk = MP.PublicKeyGenProtocol(kg)
        sk, crp, share = device_secret(rg, c, 0), pk._new(MP.PublicKeyGenCRP), pk.AllocateShare()
        n, prof = census(ctx, c, lambda: pk.GenShare(sk, crp, share))
        print(c.id, "pk_gen_share", n, {k: v[0] for k, v in prof.items() if v[0]})
        assert n == want_pk
    c = K.C_3P2
    rg = rig(ctx, c)
    prng, noise = sampling.PRNG(R.seeded_source(6).read), sampling.PRNG(R.seeded_source(7).read)
    kg = G.KeyGenerator(rg.ev, prng, M.XS_P, M.SIGMA, M.BOUND)
    sk = device_secret(rg, c, 0)
    ks = MP.KeySwitchProtocol(kg, M.CKS_NOISE_SIGMA, M.NOISE_FRESH_SK)
    pkq = M.pcks_target(c)[1]
    pub = E.PublicKey(tuple((up(rg.gQ, q), up(rg.gP, p)) for q, p in pkq))
    enc = E.Encryptor(rg.ev, prng, pub, M.XS_P, M.SIGMA, M.BOUND)
    pc = MP.PublicKeySwitchProtocol(enc, noise, M.CKS_NOISE_SIGMA, M.NOISE_FRESH_SK)
    for is_ntt in (True, False):
        ct = E.Element([rg.gQ.NewPoly(), up(rg.gQ, K.uniform_poly(c, 5))], is_ntt, False)
        share = ks.AllocateShare(c.levelQ)
        n, prof = census(ctx, c, lambda: ks.GenShare(sk, sk, ct, share))
        print("cks_gen_share ntt" if is_ntt else "cks_gen_share coefficients", n, {k: v[0] for k, v in prof.items() if v[0]})
        assert n == 6  # he_mp_cks_gen_share: 6 in both branches
        zero = E.Element([rg.gQ.NewPoly(), rg.gQ.NewPoly()], is_ntt, False)
        n0, _ = census(ctx, c, lambda: enc.EncryptZero(zero))
        pshare = pc.AllocateShare(c.levelQ)
        n, prof = census(ctx, c, lambda: pc.GenShare(sk, pub, ct, pshare))
        print("pcks_gen_share", is_ntt, n, "EncryptZero", n0, {k: v[0] for k, v in prof.items() if v[0]})
        assert n == n0 + (5 if is_ntt else 6)  # he_mp_pcks_gen_share: those of he_encrypt_zero and 5 (NTT) or 6 more
    # the finalisations: he_mp_evk_finalize copies only; he_mp_rlk_finalize is one launch in all (a key with a derived
    # double-precision copy adds its refresh, as he_evk_commit does: no key of these shapes has one)
    pr, _ = party(rg, 8)
    crp, share, key = device_crp(rg, c), pr.AllocateShare(params(c)), pr.kgen.NewEvaluationKey(params(c))
    n, prof = census(ctx, c, lambda: pr.GenEvaluationKey(share, crp, key))
    assert n == 0, prof
    n, prof = census(ctx, c, lambda: L.he_mp_rlk_finalize(crp.key.h, share.key.h, key.h))
    assert n == 1 and prof["rlk_finalize"][0] == 1
    # logN 13: the transform takes two passes, one launch more after the last draw
    cb = K.C_BIG
    rgb = rig(ctx, cb)
    prb, _ = party(rgb, 9)
    rk = MP.RelinearizationKeyGenProtocol(prb.kgen)
    crp, share = device_crp(rgb, cb), prb.AllocateShare(params(cb))
    sk0, sk1 = device_secret(rgb, cb, 0), device_secret(rgb, cb, 1)
    assert census(ctx, cb, lambda: prb.GenShare(sk0, sk1, crp, share))[0] == cb.rows + 5
    eph, r1, r2 = rk.AllocateShare(params(cb))
    agg1 = MP.RelinearizationKeyGenShare(key_of(rgb, cb, halves(M.want_rkg(cb, 1)["share1"][0], 0), halves(M.want_rkg(cb, 1)["share1"][0], 1)), 1)
    assert census(ctx, cb, lambda: rk.GenShareRoundTwo(eph, sk0, agg1, r2))[0] == cb.rows + 5
    n, prof = census(ctx, cb, lambda: rk.GenShareRoundOne(sk0, crp, eph, r1))
    print("logN 13 round one", n, {k: v[0] for k, v in prof.items() if v[0]})
    assert n == cb.rows + 5 + 9  # the ephemeral key's two transforms take two passes each as well


def test_refusals_of_the_later_entries(ctx):
    c = K.C_3P2
    rg = rig(ctx, c)
    sk = device_secret(rg, c, 0)
    pr, prng = rkg_party(rg, c, 0)
    L = la.load()
    crp = device_crp(rg, c, MP.RelinearizationKeyGenCRP)
    eph, r1, r2 = pr.AllocateShare()
    low = MP.RelinearizationKeyGenShare(pr.kgen.NewEvaluationKey(G.EvaluationKeyParameters(1, 1, 0)), 1)
    refused(lambda: pr.GenShareRoundOne(sk, crp, eph, MP.RelinearizationKeyGenShare(crp.key, 1)))  # crp and share1 one key
    refused(lambda: pr.GenShareRoundOne(sk, crp, eph, low))
    refused(lambda: pr.GenShareRoundOne(sk, crp, sk, r1))                                          # the ephemeral key is the secret key
    refused(lambda: pr.GenShareRoundOne(sk, crp, E.SecretKey(eph.Q, eph.Q), r1))
    refused(lambda: pr.GenShareRoundTwo(eph, sk, r1, r1))                                          # round1 and share2 one key
    refused(lambda: pr.GenShareRoundTwo(eph, sk, low, r2))
    refused(lambda: pr.GenRelinearizationKey(r1, low, r2.key))
    refused(lambda: pr.AggregateShares(r1, low, r1))
    pk = MP.PublicKeyGenProtocol(pr.kgen)
    pcrp, share = pk._new(MP.PublicKeyGenCRP), pk.AllocateShare()
    refused(lambda: pk.GenShare(sk, pcrp, MP.PublicKeyGenShare(sk.Q, share.P)))
    refused(lambda: pk.GenShare(sk, pcrp, MP.PublicKeyGenShare(pcrp.Q, share.P)))
    refused(lambda: pk.GenShare(sk, pcrp, MP.PublicKeyGenShare(share.Q, sk.P)))
    refused(lambda: pk.GenShare(sk, pcrp, MP.PublicKeyGenShare(share.Q, pcrp.P)))
    refused(lambda: pk.GenShare(sk, pcrp, MP.PublicKeyGenShare(share.P, share.P)))
    refused(lambda: pk.GenShare(sk, pcrp, MP.PublicKeyGenShare(rg.gQ.AtLevel(1).NewPoly(), share.P)))  # a share below the top level
    ks = MP.KeySwitchProtocol(pr.kgen, 1.0, M.SIGMA)
    c1, out = rg.gQ.NewPoly(), rg.gQ.NewPoly()
    h = lambda level, a, b, x, sigma, bound, o: la._lib.check(L.he_mp_cks_gen_share(pr.kgen.h, level, a.h, b.h, x.h, 1, sigma, bound, o.h))
    for bad in (sk.Q, c1):
        refused(lambda: h(2, sk.Q, sk.Q, c1, 3.2, 19.2, bad))      # the share is an input
    refused(lambda: h(3, sk.Q, sk.Q, c1, 3.2, 19.2, out))          # a level the ring does not have
    refused(lambda: h(2, sk.Q, sk.Q, rg.gQ.AtLevel(1).NewPoly(), 3.2, 19.2, out))  # c1 below the level
    refused(lambda: h(2, sk.Q, sk.Q, c1, 0.0, 19.2, out))
    refused(lambda: h(2, sk.Q, sk.Q, c1, 3.2, -1.0, out))
    with pytest.raises(ValueError):
        ks.AggregateShares(ks.AllocateShare(2), ks.AllocateShare(1), ks.AllocateShare(2))
    assert prng.Position() == 0 and not r1.key.download().any() and not out.download().any() and not eph.Q.download().any()
    assert {(n, a, b) for n, a, b in A.REFUSED} >= {("he_mp_rkg_round_one", "crp", "share1"), ("he_mp_rkg_round_two", "round1", "share2")}
    # inside a graph capture
    gc.collect()
    assert L.he_graph_begin(ctx.h) == 0
    try:
        codes = [L.he_mp_rkg_round_one(pr.kgen.h, sk.Q.h, sk.P.h, crp.key.h, eph.Q.h, eph.P.h, r1.key.h),
                 L.he_mp_rkg_round_two(pr.kgen.h, eph.Q.h, eph.P.h, sk.Q.h, sk.P.h, r1.key.h, r2.key.h), L.he_mp_rlk_finalize(r1.key.h, r2.key.h, r2.key.h),
                 L.he_mp_pk_gen_share(pr.kgen.h, sk.Q.h, sk.P.h, pcrp.Q.h, pcrp.P.h, share.Q.h, share.P.h),
                 L.he_mp_cks_gen_share(pr.kgen.h, 2, sk.Q.h, sk.Q.h, c1.h, 1, 3.2, 19.2, out.h)]
    finally:
        g = C.c_uint64()
        rc = L.he_graph_end(ctx.h, C.byref(g))
        assert rc == 0, L.he_last_error()
        L.he_graph_destroy(g.value)
    assert codes == [HE_EINVAL] * 5 and prng.Position() == 0
    # a failing source
    dead = sampling.PRNG(lambda n: b"")
    kg = G.KeyGenerator(rg.ev, dead)
    for call in (lambda: MP.RelinearizationKeyGenProtocol(kg).GenShareRoundOne(sk, crp, eph, r1),
                 lambda: MP.RelinearizationKeyGenProtocol(kg).GenShareRoundTwo(sk, sk, r1, r2), lambda: MP.PublicKeyGenProtocol(kg).GenShare(sk, pcrp, share),
                 lambda: MP.KeySwitchProtocol(kg, 1.0, M.SIGMA).GenShare(sk, sk, E.Element([c1, c1]), ks.AllocateShare(2)),
                 lambda: MP.PublicKeyGenProtocol(kg).SampleCRP(dead)):
        refused(call, HE_EPRNG)
        assert dead.Position() == 0
