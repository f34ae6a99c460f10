"""rlwe.KeyGenerator on the device (include/hering_keygen.h) against the restatement of the reference (tests/keygen_ref.py over the
oracle's ring operations): every word, and the position of the source afterwards.  The cases are those of tests/keygen_cases.py,
each of which has passed the host check that exp / log cannot change a word of it."""
import ctypes as C
import gc
import math
from fractions import Fraction

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd import HeringError, sampling
from lattigo_amd import encryptor as E
from lattigo_amd import keygen as G
from tests import boundary
from tests import keygen_aliasing as A
from tests import keygen_cases as K
from tests import keygen_ref as KR
from tests import sampler_ref as R
from tests.encryptor_cases import centered
from tests.gpu_common import ctx  # noqa: F401

pytestmark = pytest.mark.gpu
HE_EINVAL, HE_EPRNG = -1, -6
_RIGS = {}


class Rig:
    def __init__(self, ctx, c: K.Case):
        self.N = c.N
        self.oQ, self.oP = K.rings(c)
        self.gQ = la.Ring(ctx, c.N, c.Q, conjugate_invariant=c.ci)
        self.gP = la.Ring(ctx, c.N, c.P, conjugate_invariant=c.ci) if c.P else None
        self.ev = la.Evaluator(self.gQ, self.gP)


@pytest.fixture(scope="module", autouse=True)
def release_rigs():
    yield
    _RIGS.clear()
    gc.collect()


def rig(ctx, c: K.Case) -> Rig:
    key = (c.logN, c.Q, c.P, c.ci)
    if key not in _RIGS:
        _RIGS[key] = Rig(ctx, c)
    return _RIGS[key]


def up(ring, words):
    """[limbs][N] words (or None) as one polynomial"""
    if ring is None or words is None:
        return None
    a = np.asarray(words, dtype=np.uint64)
    return la.Poly(ring, a.shape[0], 1).upload(a[None])


def device_secret(rg: Rig, c: K.Case):
    q, p = K.secret(c)
    return E.SecretKey(up(rg.gQ, q), up(rg.gP, p))


def generator(rg: Rig, seed):
    prng = sampling.PRNG(R.seeded_source(seed).read)
    return G.KeyGenerator(rg.ev, prng, K.XS_P, K.SIGMA, K.BOUND), prng


def params(c: K.Case):
    return G.EvaluationKeyParameters(c.levelQ, c.levelP, c.pw2)


# ---- 1. word for word, position for position ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.RLK_CASES, ids=lambda c: c.id)
def test_relinearization_key(ctx, c):
    rg = rig(ctx, c)
    want, _, pos, _ = K.want_rlk(c)
    kg, prng = generator(rg, c.seed)
    rlk = kg.GenRelinearizationKeyNew(device_secret(rg, c), params(c))
    assert rlk.Shape()[:3] == (c.rows, c.levelQ + 1, c.levelP + 1)
    assert np.array_equal(rlk.download(), KR.image(want))
    assert prng.Position() == pos


@pytest.mark.parametrize("c", K.GALOIS_CASES, ids=lambda c: c.id)
def test_galois_key(ctx, c):
    rg = rig(ctx, c)
    sk = device_secret(rg, c)
    for g in K.galois_elements(c):
        want, _, pos, _ = K.want_galois(c, g)
        kg, prng = generator(rg, c.seed + 100 + g % 89)
        gk = kg.GenGaloisKeyNew(g, sk, params(c))
        assert (gk.GaloisElement, gk.NthRoot) == (g, rg.oQ.NthRoot())
        assert np.array_equal(gk.EvaluationKey.download(), KR.image(want)), g
        assert prng.Position() == pos, g
    assert np.array_equal(sk.Q.download()[0], K.secret(c)[0])


def test_galois_keys_on_one_source(ctx):
    c = K.GALOIS_SET_CASE
    rg = rig(ctx, c)
    want, _, pos, _ = K.want_galois_set(c)
    kg, prng = generator(rg, c.seed + 300)
    gks = kg.GenGaloisKeysNew(K.galois_elements(c), device_secret(rg, c), params(c))
    for gk, w in zip(gks, want):
        assert np.array_equal(gk.EvaluationKey.download(), KR.image(w)), gk.GaloisElement
    assert prng.Position() == pos


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("c", K.SK_CASES, ids=lambda c: c.id)
def test_secret_key(ctx, c, sparse):
    rg = rig(ctx, c)
    hw = K.sk_hw(c) if sparse else None
    (wq, wp), pos = K.want_sk(c, hw)
    kg, prng = generator(rg, c.seed + 400 + (hw or 0))
    sk = kg.GenSecretKeyWithHammingWeightNew(hw) if sparse else kg.GenSecretKeyNew()
    assert np.array_equal(sk.Q.download()[0], wq)
    assert (sk.P is None) == (wp is None) and (wp is None or np.array_equal(sk.P.download()[0], wp))
    assert prng.Position() == pos


@pytest.mark.parametrize("montgomery", [False, True])
@pytest.mark.parametrize("hw", [1, 8, 9, 31, 32, 37])
def test_sparse_sampler(ctx, hw, montgomery):
    c = K.C_3P2
    rg = rig(ctx, c)
    src = R.seeded_source(900 + hw)
    want = KR.sample_sparse(src, c.N, c.Q[:2], hw, montgomery)
    prng = sampling.PRNG(R.seeded_source(900 + hw).read)
    pol = rg.gQ.NewPoly()
    pol.upload(np.full((1, 3, c.N), 0x5555, dtype=np.uint64))
    G.SparseTernarySampler(prng, rg.gQ, hw, montgomery).AtLevel(1).Read(pol)
    got = pol.download()[0]
    assert np.array_equal(got[:2], np.array(want, dtype=np.uint64)) and np.all(got[2] == 0x5555)
    assert prng.Position() == src.pos


@pytest.mark.parametrize("up_", [True, False], ids=["small-to-large", "large-to-small"])
def test_evaluation_key_between_ring_degrees(ctx, up_):
    c = K.C_SWITCH
    rg = rig(ctx, c)
    want, _, pos, _ = K.want_switch(c, up_)
    small_ring = la.Ring(ctx, 1 << K.SMALL_LOGN, c.Q)
    small, large = E.SecretKey(up(small_ring, K.small_secret(c))), device_secret(rg, c)
    kg, prng = generator(rg, c.seed + 500 + int(up_))
    evk = kg.GenEvaluationKeyNew(*((small, large) if up_ else (large, small)), params(c))
    assert np.array_equal(evk.download(), KR.image(want))
    assert prng.Position() == pos


# ---- 2. fused against composed --------------------------------------------------------------------------------------------------------
def composed_key(rg: Rig, c: K.Case, prng, skIn, skOut):
    """the same key from the public entries: Encryptor.EncryptZero on each row, then he_gadget_add_poly"""
    enc = E.Encryptor(rg.ev, prng, skOut, K.XS_P, K.SIGMA, K.BOUND)
    rq, rp = rg.gQ.AtLevel(c.levelQ), (rg.gP.AtLevel(c.levelP) if c.levelP >= 0 else None)
    q = np.zeros((c.rows, 2, c.levelQ + 1, c.N), dtype=np.uint64)
    p = np.zeros((c.rows, 2, c.levelP + 1, c.N), dtype=np.uint64)
    for r in range(c.rows):
        ct = E.ElementQP([(rq.NewPoly(), rp.NewPoly() if rp is not None else None) for _ in range(2)], True, True, c.levelQ, c.levelP)
        enc.EncryptZero(ct)
        for k in range(2):
            q[r, k] = ct.Value[k][0].download()[0]
            if rp is not None:
                p[r, k] = ct.Value[k][1].download()[0]
    nj = KR.base_two_sizes(c.Q, c.levelQ, c.levelP, c.pw2) if c.pw2 else None
    key = rg.ev.NewEvaluationKey(q, p if c.levelP >= 0 else None, c.pw2, nj)
    G.AddPolyTimesGadgetVectorToGadgetCiphertext(skIn, [key])
    return key


@pytest.mark.parametrize("c", [K.C_3P2, K.C_LOW, K.C_B16, K.C_B16_NOP], ids=lambda c: c.id)
def test_fused_equals_composed(ctx, c):
    rg = rig(ctx, c)
    sk = device_secret(rg, c)
    skIn = up(rg.gQ, K.uniform_poly(c, 3))
    kg, prng = generator(rg, c.seed + 700)
    fused = kg.NewEvaluationKey(params(c))
    kg.genEvaluationKey(skIn, sk, fused)
    prng2 = sampling.PRNG(R.seeded_source(c.seed + 700).read)
    composed = composed_key(rg, c, prng2, skIn, sk)
    assert np.array_equal(fused.download(), composed.download())
    assert prng.Position() == prng2.Position() > 0


# ---- 3. the gadget term alone -----------------------------------------------------------------------------------------------------------
def filled_key(rg: Rig, c: K.Case, kind, rng):
    q = np.stack([[[boundary.word_row(kind, rng, m, c.N) for m in c.Q[:c.levelQ + 1]] for _ in range(2)] for _ in range(c.rows)])
    p = np.stack([[[boundary.word_row(kind, rng, m, c.N) for m in c.P[:c.levelP + 1]] for _ in range(2)] for _ in range(c.rows)]) if c.levelP >= 0 else None
    nj = KR.base_two_sizes(c.Q, c.levelQ, c.levelP, c.pw2) if c.pw2 else None
    return rg.ev.NewEvaluationKey(q, p, c.pw2, nj), q, p


@pytest.mark.parametrize("c", K.GADGET_CASES, ids=lambda c: c.id)
def test_gadget_add_poly(ctx, c):
    """on keys of worst-case canonical words, one key and two: the term lands on component u of key u, on the limbs of the row's
    own digit, and nothing else moves"""
    rg = rig(ctx, c)
    rng = np.random.default_rng(c.seed)
    pt = K.uniform_poly(c, 4)
    dpt = up(rg.gQ, pt)
    for kind in ("max", "alt", "half"):
        (k0, q0, p0), (k1, q1, p1) = filled_key(rg, c, kind, rng), filled_key(rg, c, "uniform", rng)
        w0, w1 = q0.copy(), q1.copy()
        KR.add_poly_times_gadget_vector(rg.oQ, rg.oP, pt, [w0, w1], c.levelQ, c.levelP, c.pw2)
        G.AddPolyTimesGadgetVectorToGadgetCiphertext(dpt, [k0, k1])
        for k, w, p in ((k0, w0, p0), (k1, w1, p1)):
            got = k.download()
            assert np.array_equal(got[:, :, :c.levelQ + 1], w), kind
            assert p is None or np.array_equal(got[:, :, c.levelQ + 1:], p), kind
        assert not np.array_equal(w0, q0) and np.array_equal(w0[:, 1], q0[:, 1]) and np.array_equal(w1[:, 0], q1[:, 0])
        one = q0.copy()  # the one-ciphertext form, on a key of the same words (these kinds draw nothing)
        KR.add_poly_times_gadget_vector(rg.oQ, rg.oP, pt, [one], c.levelQ, c.levelP, c.pw2)
        k2, _, _ = filled_key(rg, c, kind, rng)
        G.AddPolyTimesGadgetVectorToGadgetCiphertext(dpt, [k2])
        assert np.array_equal(k2.download()[:, :, :c.levelQ + 1], one), kind
    assert np.array_equal(dpt.download()[0], pt)


# ---- 4. a generated key behaves as the same words uploaded --------------------------------------------------------------------------------
def test_generated_key_behaves_as_uploaded(ctx):
    """on the class chain, whose limb below 2^47 gives the key its derived double-precision copy"""
    c = K.C_CLASS
    rg = rig(ctx, c)
    kg, _ = generator(rg, c.seed)
    rlk = kg.GenRelinearizationKeyNew(device_secret(rg, c), params(c))
    img = rlk.download()
    again = rg.ev.NewEvaluationKey(img[:, :, :c.levelQ + 1], img[:, :, c.levelQ + 1:])
    cx = up(rg.gQ, K.uniform_poly(c, 6))
    outs = []
    for key in (rlk, again):
        ct = [rg.gQ.NewPoly(), rg.gQ.NewPoly()]
        rg.ev.GadgetProduct(c.levelQ, cx, key, ct)
        outs.append([x.download() for x in ct])
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and outs[0][0].any()


# ---- 5. end to end on the device, from one seeded source ---------------------------------------------------------------------------------
def crt_centered(words, moduli):
    """[limbs][N] canonical words -> the centred integers modulo the product"""
    M = math.prod(moduli)
    out = []
    for j in range(words.shape[1]):
        x = 0
        for i, q in enumerate(moduli):
            Mi = M // q
            x += int(words[i][j]) * Mi * pow(Mi, -1, q)
        x %= M
        out.append(x - M if x > M // 2 else x)
    return out


def negacyclic_auto(m, g):
    """X^i -> X^(i g) on Z[X]/(X^N + 1)"""
    N = len(m)
    out = [0] * N
    for i, v in enumerate(m):
        k = i * g % (2 * N)
        if k < N:
            out[k] += v
        else:
            out[k - N] -= v
    return out


def test_end_to_end_from_one_source(ctx):
    """GenSecretKey -> GenPublicKey -> a relinearization key and Galois keys for 5 and NthRoot - 1, all on the device from one source;
    then Relinearize of a noiseless degree-2 ciphertext of Delta m (built on the oracle from the downloaded secret key) and Automorphism
    of a ciphertext of Delta m encrypted under pk on the device; Decrypt on the device.  m and its automorphisms come back exactly.

    The worst-case noise, N = 64, Q of 4 limbs, P of 2 limbs, beta = 2, every Gaussian |e| <= 19, the secret and u ternary:
      fresh under pk (encryptZeroPk on a ring.Poly element: QP at levelP = 0, then ModDown by p_0):
          |u e_pk + e0 + e1 s| <= 19 (2 N + 1), divided by p_0, plus the ModDown rounding (1/2 on c0, 1/2 on c1 times s: (1 + N) / 2);
      a key switch (Relinearize, Automorphism): sum over the beta digits of <digit_i(c), e_i>, each digit below D_i = the product of its
          Q limbs, N terms each: <= beta N 19 max(D_i), divided by P, plus the ModDown rounding (1 + N) / 2.
    An automorphism permutes the fresh noise and adds one key switch; Relinearize of a noiseless ciphertext adds one key switch.  So
    B = 19 (2 N + 1) / p_0 + (1 + N) / 2 + beta N 19 max(D_i) / P + (1 + N) / 2 bounds both, about 2.5e3; Delta = 2^40 >= 4 B."""
    c = K.C_4P2
    rg = rig(ctx, c)
    N, Q, P = c.N, c.Q, c.P
    alpha, beta = len(P), KR.base_rns_size(c.levelQ, c.levelP)
    Dmax = max(math.prod(Q[i * alpha:(i + 1) * alpha]) for i in range(beta))
    B = Fraction(19 * (2 * N + 1), P[0]) + Fraction(1 + N, 2) + Fraction(beta * N * 19 * Dmax, math.prod(P)) + Fraction(1 + N, 2)
    Delta = 1 << 40
    assert 4 * B <= Delta and Delta * (1 << 16) * 4 < math.prod(Q)
    kg, prng = generator(rg, 4242)
    sk, pk = kg.GenKeyPairNew()
    rlk = kg.GenRelinearizationKeyNew(sk)
    nth = rg.oQ.NthRoot()
    gks = kg.GenGaloisKeysNew([5, nth - 1], sk)
    assert prng.Position() > 0
    rng = np.random.default_rng(17)
    m = [int(x) for x in rng.integers(0, 1 << 16, N)]
    oQ = rg.oQ
    dm = oQ.NTT(np.stack([np.array([Delta * x % q for x in m], dtype=np.uint64) for q in Q]))
    dec = E.Decryptor(rg.ev, sk)

    def decrypt(ct):
        pt = E.Plaintext(rg.gQ.NewPoly())
        dec.Decrypt(E.Element(ct, True, False), pt)
        return crt_centered(oQ.INTT(pt.Value.download()[0]), Q)

    def check(ct, want, what):
        got = decrypt(ct)
        noise = max(abs(g - Delta * w) for g, w in zip(got, want))
        print(what, "noise", noise, "bound", float(B))
        assert [(g + Delta // 2) // Delta for g in got] == want, what
        assert noise <= B, what

    # Relinearize: c0 + c1 s + c2 s^2 = Delta m, exactly
    skQ = sk.Q.download()[0]
    c1, c2 = K.uniform_poly(c, 8), K.uniform_poly(c, 9)
    s2 = oQ.binop("MulCoeffsMontgomery", skQ, skQ)
    c0 = oQ.binop("Sub", oQ.binop("Sub", dm, oQ.binop("MulCoeffsMontgomery", c1, skQ)), oQ.binop("MulCoeffsMontgomery", c2, s2))
    out = [rg.gQ.NewPoly(), rg.gQ.NewPoly()]
    rg.ev.Relinearize(c.levelQ, [up(rg.gQ, x) for x in (c0, c1, c2)], rlk, out)
    check(out, m, "relinearize")
    # Automorphism of a ciphertext encrypted under pk on the device
    ct = E.Element([rg.gQ.NewPoly(), rg.gQ.NewPoly()])
    E.Encryptor(rg.ev, prng, pk, K.XS_P, K.SIGMA, K.BOUND).Encrypt(E.Plaintext(up(rg.gQ, dm), True, False), ct)
    check(ct.Value, m, "fresh")
    for gk in gks:
        out = [rg.gQ.NewPoly(), rg.gQ.NewPoly()]
        rg.ev.Automorphism(c.levelQ, ct.Value, gk.GaloisElement, gk.EvaluationKey, out)
        check(out, negacyclic_auto(m, gk.GaloisElement), f"automorphism {gk.GaloisElement}")


# ---- 6. launches -------------------------------------------------------------------------------------------------------------------------
def census(ctx, c: K.Case, composed: bool):
    rg = rig(ctx, c)
    sk = device_secret(rg, c)
    kg, prng = generator(rg, c.seed + 800)
    evk = kg.NewEvaluationKey(params(c))
    kg.genEvaluationKey(sk.Q, sk, evk)  # (once outside: the scratch has its size)
    if composed:
        composed_key(rg, c, prng, sk.Q, sk)
    ctx.sync()
    ctx.prof_begin()
    if composed:
        composed_key(rg, c, prng, sk.Q, sk)
    else:
        kg.genEvaluationKey(sk.Q, sk, evk)
    ctx.sync()
    prof = ctx.prof_end()
    return sum(v[0] for v in prof.values()), prof


def test_launch_census(ctx):
    """he_keygen_evaluation_key: the same launches at logN 6 and logN 8 and at two levels, at most 3 R + 8 for R rows, two per row,
    and fewer than the composed loop's"""
    shapes = [K.C_4P2, K.C_LOW, K._case("census-logN8", 8, K.C_4P2.Q, K.C_4P2.P, 230)]
    counts = {}
    for c in shapes:
        n, prof = census(ctx, c, False)
        print(c.id, "rows", c.rows, "launches", n, {k: v[0] for k, v in prof.items()})
        assert n <= 3 * c.rows + 8
        assert prof["evk_finish"][0] == 1 and prof["sampler_uniform"][0] == prof["sampler_gaussian"][0] == c.rows
        counts[c.id] = n - 2 * c.rows  # the launches after the last draw
    assert len(set(counts.values())) == 1, counts
    assert census(ctx, K.C_4P2, False)[0] == census(ctx, shapes[2], False)[0]
    n_composed, prof = census(ctx, K.C_4P2, True)
    print("composed", n_composed, {k: v[0] for k, v in prof.items()})
    assert census(ctx, K.C_4P2, False)[0] < n_composed


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def refused(call, code=HE_EINVAL):
    with pytest.raises(HeringError) as e:
        call()
    assert e.value.code == code, e.value


def test_refusals_touch_nothing(ctx):
    c = K.C_3P2
    rg = rig(ctx, c)
    sk = device_secret(rg, c)
    kg, prng = generator(rg, 1)
    good = kg.NewEvaluationKey()
    refused(lambda: kg.genEvaluationKey(sk.Q, sk, la.EvaluationKey(rg.ev, None, None, shape=(3, 3, 2))))  # beta against the levels
    other = Rig(ctx, c)
    refused(lambda: kg.GenRelinearizationKey(sk, la.EvaluationKey(other.ev, None, None, shape=(2, 3, 2))))  # a key of another evaluator
    sk3 = E.SecretKey(rg.gQ.NewPoly(3), rg.gP.NewPoly(3))
    refused(lambda: kg.GenRelinearizationKey(sk3, good))  # a batch-3 secret key
    refused(lambda: kg.GenGaloisKey(4, sk, good))  # an even Galois element
    refused(lambda: kg.GenGaloisKeys([5, 6], sk, [good, kg.NewEvaluationKey()]))
    refused(lambda: kg.GenSecretKeyWithHammingWeightNew(0))
    refused(lambda: kg.GenSecretKeyWithHammingWeightNew(-3))
    refused(lambda: G.SparseTernarySampler(prng, rg.gQ, 0, False).ReadNew())
    # an output that is a key operand or another output: the pairs of tests/keygen_aliasing.py
    assert sorted(n for n, _, _ in A.PAIRS) == sorted(n for n, r in A.ROWS.items() if sum(r.written(p) for p in r.params) > 1 or r.arrays)
    one = la.Poly(rg.gQ, 3)
    refused(lambda: kg.GenSecretKey(E.SecretKey(one, one)))
    refused(lambda: kg.GenSecretKeyWithHammingWeight(5, E.SecretKey(one, one)))
    refused(lambda: G.AddPolyTimesGadgetVectorToGadgetCiphertext(sk.Q, [good, good]))
    refused(lambda: kg.GenGaloisKeys([5, 13], sk, [good, good]))
    assert prng.Position() == 0 and not good.download().any()
    # a conjugate-invariant ring has the automorphisms 5^k alone
    ci = rig(ctx, K.C_CI)
    kgci, prngci = generator(ci, 2)
    refused(lambda: kgci.GenGaloisKeyNew(ci.oQ.NthRoot() - 1, device_secret(ci, K.C_CI)))
    assert prngci.Position() == 0


def test_refused_inside_a_graph_capture(ctx):
    c = K.C_3P2
    rg = rig(ctx, c)
    sk = device_secret(rg, c)
    kg, prng = generator(rg, 3)
    evk = kg.NewEvaluationKey()
    kg.genEvaluationKey(sk.Q, sk, evk)  # (once outside, as a capture asks)
    pos, img = prng.Position(), evk.download()
    L = la.load()
    assert L.he_graph_begin(ctx.h) == 0
    try:
        for call in (lambda: kg.genEvaluationKey(sk.Q, sk, evk), lambda: kg.GenRelinearizationKey(sk, evk), lambda: kg.GenGaloisKey(5, sk, evk),
                     lambda: kg.GenGaloisKeys([5], sk, [evk]), lambda: kg.GenEvaluationKey(sk, sk, evk), lambda: kg.GenSecretKey(sk),
                     lambda: kg.GenSecretKeyWithHammingWeight(4, sk), lambda: G.SparseTernarySampler(prng, rg.gQ, 4, False).Read(sk.Q),
                     lambda: G.AddPolyTimesGadgetVectorToGadgetCiphertext(sk.Q, [evk])):
            refused(call)
    finally:
        g = C.c_uint64()
        assert L.he_graph_end(ctx.h, C.byref(g)) == 0
        L.he_graph_destroy(g.value)
    assert prng.Position() == pos and np.array_equal(evk.download(), img)


def test_a_failing_source_is_eprng_and_consumes_nothing(ctx):
    c = K.C_3P2
    rg = rig(ctx, c)
    sk = device_secret(rg, c)
    prng = sampling.PRNG(lambda n: b"")  # a short read
    kg = G.KeyGenerator(rg.ev, prng)
    evk = kg.NewEvaluationKey()
    for call in (lambda: kg.GenRelinearizationKey(sk, evk), lambda: kg.GenGaloisKey(5, sk, evk), lambda: kg.GenSecretKeyNew(),
                 lambda: kg.GenSecretKeyWithHammingWeightNew(7), lambda: kg.GenEvaluationKey(sk, sk, evk)):
        refused(call, HE_EPRNG)
        assert prng.Position() == 0
