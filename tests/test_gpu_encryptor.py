"""rlwe.Encryptor / rlwe.Decryptor on the device (include/hering_encryptor.h) against the restatement of the reference
(tests/encryptor_ref.py over the oracle's ring operations): every word, and the position of the source afterwards.  The cases are
those of tests/encryptor_cases.py, each of which has passed the host check that exp / log cannot change a word of it."""
import ctypes as C
import gc

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd import HeringError, bgv, ckks, sampling
from lattigo_amd import encryptor as E
from tests import encryptor_aliasing as A
from tests import encryptor_cases as K
from tests import encryptor_ref as ER
from tests import sampler_ref as R
from tests.conftest import Pi60, Qi60
from tests.gpu_common import ctx  # noqa: F401

pytestmark = pytest.mark.gpu
HE_EINVAL = -1
_RIGS = {}


class Rig:
    def __init__(self, ctx, logN, nq, npp):
        self.N = 1 << logN
        self.oQ, self.oP = K.rings(logN, nq, npp)
        self.gQ = la.Ring(ctx, self.N, Qi60[:nq])
        self.gP = la.Ring(ctx, self.N, Pi60[:npp]) if npp else None
        self.ev = la.Evaluator(self.gQ, self.gP)


@pytest.fixture(scope="module", autouse=True)
def release_rigs():
    yield
    _RIGS.clear()
    gc.collect()


def rig(ctx, logN, nq, npp) -> Rig:
    key = (logN, nq, npp)
    if key not in _RIGS:
        _RIGS[key] = Rig(ctx, logN, nq, npp)
    return _RIGS[key]


def up(ring, entries):
    """[entry][limbs][N] words (or None) as one polynomial of that batch"""
    if ring is None or entries[0] is None:
        return None
    a = np.stack(entries)
    return la.Poly(ring, a.shape[1], a.shape[0]).upload(a)


def device_key(rg: Rig, c: K.Case):
    ks = K.keys(c)
    if c.key == "sk":
        return E.SecretKey(up(rg.gQ, [k[0] for k in ks]), up(rg.gP, [k[1] for k in ks]))
    return E.PublicKey(tuple((up(rg.gQ, [k[i][0] for k in ks]), up(rg.gP, [k[i][1] for k in ks])) for i in range(2)))


def filled(ring, batch, word=0x5555):
    """an output that holds other words before the call"""
    p = ring.NewPoly(batch)
    p.upload(np.full((batch, p.n_limbs, p.N), word, dtype=np.uint64))
    return p


def element_for(rg: Rig, c: K.Case, is_ntt, is_mont):
    if c.qp:
        return E.ElementQP([(filled(rg.gQ, c.batch), filled(rg.gP, c.batch)) for _ in range(2)], bool(is_ntt), bool(is_mont), c.levelQ, c.levelP)
    return E.Element([filled(rg.gQ, c.batch) for _ in range(2)], bool(is_ntt), bool(is_mont), c.levelQ)


def assert_zero_equals(c: K.Case, ct, want):
    for k in range(2):
        q, p = (ct.Value[k] if c.qp else (ct.Value[k], None))
        got = q.download()
        assert np.array_equal(got[:, :c.levelQ + 1], np.stack([e[k][0] for e in want])), ("Q", k)
        assert np.all(got[:, c.levelQ + 1:] == 0x5555), "limbs above the level are left alone"
        if c.qp:
            got = p.download()
            assert np.array_equal(got[:, :c.levelP + 1], np.stack([e[k][1] for e in want])), ("P", k)
            assert np.all(got[:, c.levelP + 1:] == 0x5555)


# ---- EncryptZero -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_ntt,is_mont", K.FLAGS)
@pytest.mark.parametrize("c", K.ZERO_CASES, ids=lambda c: c.id)
def test_encrypt_zero(ctx, c, is_ntt, is_mont):
    rg = rig(ctx, c.logN, c.nq, c.npp)
    want, pos = K.want_zero(c, is_ntt, is_mont)
    prng = sampling.PRNG(R.seeded_source(c.seed).read)
    enc = E.Encryptor(rg.ev, prng, device_key(rg, c), K.XS_P, K.SIGMA, K.BOUND)
    ct = element_for(rg, c, is_ntt, is_mont)
    enc.EncryptZero(ct)
    assert_zero_equals(c, ct, want)
    assert prng.Position() == pos


def test_calls_stay_in_step_and_with_key_rebinds(ctx):
    """two calls on one source, the second under another key through WithKey: the second starts where the first ended (the sequence
    of tests/encryptor_cases.py, which has passed the host check as a whole)"""
    c1, c2 = K.SEQUENCE
    rg = rig(ctx, c1.logN, c1.nq, c1.npp)
    (w1, w2), pos = K.run_sequence()
    prng = sampling.PRNG(R.seeded_source(K.SEQUENCE_SEED).read)
    enc = E.Encryptor(rg.ev, prng, device_key(rg, c1), K.XS_P, K.SIGMA, K.BOUND)
    ct1, ct2 = element_for(rg, c1, 1, 0), element_for(rg, c2, 1, 0)
    enc.EncryptZero(ct1)
    enc.WithKey(device_key(rg, c2)).EncryptZero(ct2)
    assert_zero_equals(c1, ct1, w1)
    assert_zero_equals(c2, ct2, w2)
    assert prng.Position() == pos
    with pytest.raises(HeringError) as e:
        E.Encryptor(rg.ev, prng).EncryptZero(ct1)  # no key
    assert e.value.code == HE_EINVAL


def test_a_secret_key_without_its_p_part(ctx):
    """with special primes, sk bound as (Q, None) serves the ring.Poly form, which reads sk.Value.Q only, with the words of the
    full key; the QP form, which reads the P part, is refused before anything is drawn"""
    c = K.ZERO_CASES[1]
    rg = rig(ctx, c.logN, c.nq, c.npp)
    want, pos = K.want_zero(c, 1, 0)
    prng = sampling.PRNG(R.seeded_source(c.seed).read)
    enc = E.Encryptor(rg.ev, prng, E.SecretKey(device_key(rg, c).Q, None), K.XS_P, K.SIGMA, K.BOUND)
    with pytest.raises(HeringError) as e:
        enc.EncryptZero(E.ElementQP([(rg.gQ.NewPoly(c.batch), rg.gP.NewPoly(c.batch)) for _ in range(2)]))
    assert e.value.code == HE_EINVAL and prng.Position() == 0
    ct = element_for(rg, c, 1, 0)
    enc.EncryptZero(ct)
    assert_zero_equals(c, ct, want)
    assert prng.Position() == pos


def test_an_exception_of_the_reader_is_the_cause_of_the_error(ctx):
    c = K.ZERO_CASES[1]
    rg = rig(ctx, c.logN, c.nq, c.npp)

    def read(n):
        raise ValueError("no more bytes")
    prng = sampling.PRNG(read)
    enc = E.Encryptor(rg.ev, prng, device_key(rg, c))
    for call in (lambda: enc.EncryptZero(element_for(rg, c, 1, 0)), lambda: sampling.GaussianSampler(prng, rg.gQ, 3.2, 19.2, False).ReadNew()):
        with pytest.raises(HeringError) as e:
            call()
        assert e.value.code == -6 and isinstance(e.value.__cause__, ValueError) and prng.error is None


# ---- Encrypt and addPtToCt -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pt_is_ntt", [1, 0])
@pytest.mark.parametrize("c", K.ENCRYPT_CASES, ids=lambda c: c.id)
def test_encrypt(ctx, c, pt_is_ntt):
    """the ciphertext takes the plaintext's metadata; level = min(pt.Level(), ct.Level()) with the plaintext one limb above it"""
    rg = rig(ctx, c.logN, c.nq, c.npp)
    rng = np.random.default_rng(c.seed)
    ptw = [K.uniform(rng, rg.oQ.moduli[:c.levelQ + 2], rg.N) for _ in range(c.batch)]
    want, pos = K.want_zero(c, pt_is_ntt, 0)
    ref = ER.Encryptor(rg.oQ, rg.oP, R.seeded_source(0))
    want0 = np.stack([ref.add_pt_to_ct(c.levelQ, ptw[b], pt_is_ntt, want[b][0][0], pt_is_ntt) for b in range(c.batch)])
    prng = sampling.PRNG(R.seeded_source(c.seed).read)
    enc = E.Encryptor(rg.ev, prng, device_key(rg, c), K.XS_P, K.SIGMA, K.BOUND)
    pt = E.Plaintext(up(rg.gQ, ptw), bool(pt_is_ntt), False)
    ct = E.Element([filled(rg.gQ, c.batch) for _ in range(2)], not pt_is_ntt, True, c.levelQ)
    enc.Encrypt(pt, ct)
    assert (ct.IsNTT, ct.IsMontgomery, ct.Level()) == (bool(pt_is_ntt), False, c.levelQ)
    assert np.array_equal(ct.Value[0].download()[:, :c.levelQ + 1], want0)
    assert np.array_equal(ct.Value[1].download()[:, :c.levelQ + 1], np.stack([e[1][0] for e in want]))
    assert prng.Position() == pos


@pytest.mark.parametrize("pt_is_ntt,ct_is_ntt", [(1, 1), (1, 0), (0, 1), (0, 0)])
@pytest.mark.parametrize("batch", [1, 3])
def test_add_pt_to_ct(ctx, pt_is_ntt, ct_is_ntt, batch):
    rg = rig(ctx, 6, 3, 2)
    rng = np.random.default_rng(5)
    ptw, c0w = ([K.uniform(rng, rg.oQ.moduli, rg.N) for _ in range(batch)] for _ in range(2))
    ref = ER.Encryptor(rg.oQ, rg.oP, R.seeded_source(0))
    prng = sampling.PRNG(R.seeded_source(0).read)
    enc = E.Encryptor(rg.ev, prng)
    pt, ct = E.Plaintext(up(rg.gQ, ptw), bool(pt_is_ntt)), E.Element([up(rg.gQ, c0w), None], bool(ct_is_ntt))
    enc.addPtToCt(1, pt, ct)
    got = ct.Value[0].download()
    assert np.array_equal(got[:, :2], np.stack([ref.add_pt_to_ct(1, ptw[b], pt_is_ntt, c0w[b], ct_is_ntt) for b in range(batch)]))
    assert np.array_equal(got[:, 2:], np.stack(c0w)[:, 2:]) and np.array_equal(pt.Value.download(), np.stack(ptw)) and prng.Position() == 0


# ---- GenPublicKey ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.GENPK_CASES, ids=lambda c: c.id)
def test_gen_public_key(ctx, c):
    rg = rig(ctx, c.logN, c.nq, c.npp)
    want, pos = K.want_zero(c, 1, 1)
    prng = sampling.PRNG(R.seeded_source(c.seed).read)
    pk = E.KeyGenerator(rg.ev, prng, K.XS_P, K.SIGMA, K.BOUND).GenPublicKeyNew(device_key(rg, c))
    for k in range(2):
        assert np.array_equal(pk.Value[k][0].download(), np.stack([e[k][0] for e in want]))
        assert np.array_equal(pk.Value[k][1].download(), np.stack([e[k][1] for e in want]))
    assert prng.Position() == pos


# ---- Decrypt -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_ntt", [1, 0])
@pytest.mark.parametrize("degree,ct_level,pt_level,batch", [(1, 2, 2, 1), (2, 2, 1, 3), (8, 2, 2, 1), (8, 1, 2, 3), (7, 2, 0, 1), (0, 2, 2, 1)])
def test_decrypt(ctx, degree, ct_level, pt_level, batch, is_ntt):
    """degree 8 passes the Reduce at i & 7 == 7; degree 7 skips the one after the loop, which in the coefficient domain is where the
    reference's INTT is not exact and the device returns the canonical decryption (include/hering_encryptor.h; the host test
    holds that form against the NTT-domain Horner value); pt.Level() below and above ct.Level()"""
    rg = rig(ctx, 6, 3, 2)
    rng = np.random.default_rng(degree * 10 + batch)
    skw = [K.uniform(rng, rg.oQ.moduli, rg.N) for _ in range(batch)]
    ctw = [[K.uniform(rng, rg.oQ.moduli, rg.N) for _ in range(batch)] for _ in range(degree + 1)]
    level = min(ct_level, pt_level)
    want = np.stack([ER.decrypt(rg.oQ, skw[b], [ctw[i][b] for i in range(degree + 1)], ct_level, pt_level, is_ntt,
                                reduce_always=not is_ntt and degree & 7 == 7)[0] for b in range(batch)])
    dec = E.Decryptor(rg.ev, E.SecretKey(up(rg.gQ, skw)))
    ct = E.Element([up(rg.gQ, ctw[i]) for i in range(degree + 1)], bool(is_ntt), False, ct_level)
    pt = E.Plaintext(filled(rg.gQ, batch), not is_ntt, True, pt_level)
    dec.Decrypt(ct, pt)
    got = pt.Value.download()
    assert (pt.IsNTT, pt.IsMontgomery, pt.Level()) == (bool(is_ntt), False, level)
    assert np.array_equal(got[:, :level + 1], want) and np.all(got[:, level + 1:] == 0x5555)
    for i in range(degree + 1):
        assert np.array_equal(ct.Value[i].download(), np.stack(ctw[i]))


# ---- end to end, on the device only ------------------------------------------------------------------------------------------------
def real_keys(rg: Rig, prng, seed):
    s, skQ, skP = K.ternary_secret(np.random.default_rng(seed), rg.oQ, rg.oP)
    sk = E.SecretKey(up(rg.gQ, [skQ]), up(rg.gP, [skP]))
    return sk, E.KeyGenerator(rg.ev, prng).GenPublicKeyNew(sk)


@pytest.mark.parametrize("npp", [2, 0])
def test_bgv_end_to_end(ctx, npp):
    """encode -> Encrypt (sk and pk) -> Decrypt -> decode gives the slots exactly"""
    T, logN = 65537, 10
    rg = rig(ctx, logN, 3, npp)
    enc_t = bgv.Encoder(rg.gQ, la.Ring(ctx, rg.N, [T]), rg.gP)
    prng = sampling.PRNG(R.seeded_source(900 + npp).read)
    sk, pk = real_keys(rg, prng, 11)
    values = np.random.default_rng(12).integers(0, T, rg.N, dtype=np.uint64)
    pt = E.Plaintext(enc_t.Encode(values, la.Poly(rg.gQ, 3, zero=False)), True, False)
    dec = E.Decryptor(rg.ev, sk)
    for key in (sk, pk):
        ct = E.Element([rg.gQ.NewPoly(), rg.gQ.NewPoly()])
        E.Encryptor(rg.ev, prng, key).Encrypt(pt, ct)
        assert not np.array_equal(ct.Value[0].download(), pt.Value.download())
        out = E.Plaintext(rg.gQ.NewPoly())
        dec.Decrypt(ct, out)
        assert np.array_equal(enc_t.Decode(out.Value)[0], values), type(key).__name__


def test_ckks_end_to_end(ctx):
    """the reference's own criterion (schemes/ckks/ckks_test.go:278-283): log2(1 / mean |error|) >= log2(scale) - (logN + 2)"""
    logN, scale = 10, float(1 << 45)
    rg = rig(ctx, logN, 3, 2)
    ecd = ckks.Encoder(rg.gQ, rg.gP)
    prng = sampling.PRNG(R.seeded_source(950).read)
    sk, pk = real_keys(rg, prng, 13)
    rng = np.random.default_rng(14)
    values = rng.uniform(-1, 1, rg.N // 2) + 1j * rng.uniform(-1, 1, rg.N // 2)
    pt = E.Plaintext(ecd.Encode(values, la.Poly(rg.gQ, 3, zero=False), Scale=scale), True, False)
    dec = E.Decryptor(rg.ev, sk)
    for key in (sk, pk):
        ct = E.Element([rg.gQ.NewPoly(), rg.gQ.NewPoly()])
        E.Encryptor(rg.ev, prng, key).Encrypt(pt, ct)
        out = E.Plaintext(rg.gQ.NewPoly())
        dec.Decrypt(ct, out)
        got = ecd.Decode(out.Value, Scale=scale)[0]
        meanprec = float(np.abs(got - values).mean())
        print(type(key).__name__, "log2(1/err) =", np.log2(1 / meanprec))
        assert np.log2(1 / meanprec) >= np.log2(scale) - (logN + 2), type(key).__name__


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_aliasing_refusals(ctx):
    """every pair of tests/encryptor_aliasing.py with an output in it, as one handle: HE_EINVAL, the source where it was"""
    rg = rig(ctx, 6, 3, 2)
    prng = sampling.PRNG(R.seeded_source(1).read)
    mk = lambda: rg.gQ.NewPoly()
    mkp = lambda: rg.gP.NewPoly()
    for name, row in A.ROWS.items():
        for a, b in A.refused_pairs(row):
            ops = {p: (mkp() if row.side(p) == "P" else mk()) for p in row.params}
            shared = mk() if "P" not in (row.side(a), row.side(b)) else la.Poly(rg.gQ, 3)
            ops[a] = ops[b] = shared
            sk = E.SecretKey(ops["key"], mkp()) if "key" in ops else None
            enc = E.Encryptor(rg.ev, prng, sk if name != "he_decryptor_decrypt" else None)
            with pytest.raises(HeringError) as e:
                if name == "he_encrypt_zero":
                    enc.EncryptZero(E.Element([ops["c0"], ops["c1"]]))
                elif name == "he_encrypt_zero_qp":
                    enc.EncryptZero(E.ElementQP([(ops["c0Q"], ops["c0P"]), (ops["c1Q"], ops["c1P"])], levelQ=2, levelP=1))
                elif name == "he_add_pt_to_ct":
                    enc.addPtToCt(2, E.Plaintext(ops["pt"]), E.Element([ops["c0"], None]))
                elif name == "he_encrypt":
                    enc.Encrypt(E.Plaintext(ops["pt"]), E.Element([ops["c0"], ops["c1"]]))
                else:
                    E.Decryptor(rg.ev, sk).Decrypt(E.Element([mk(), ops["ct"]]), E.Plaintext(ops["pt"]))
            assert e.value.code == HE_EINVAL, (name, a, b)
    assert prng.Position() == 0


def test_refused_inside_a_graph_capture(ctx):
    rg = rig(ctx, 6, 3, 2)
    c = K.ZERO_CASES[1]
    prng = sampling.PRNG(R.seeded_source(2).read)
    enc = E.Encryptor(rg.ev, prng, device_key(rg, c))
    dec = E.Decryptor(rg.ev, E.SecretKey(rg.gQ.NewPoly(3)))
    ct, pt = element_for(rg, c, 1, 0), E.Plaintext(rg.gQ.NewPoly(3))
    enc.EncryptZero(ct)  # (once outside, as a capture asks)
    pos = prng.Position()
    load = la.load()
    assert load.he_graph_begin(ctx.h) == 0
    try:
        for call in (lambda: enc.EncryptZero(ct), lambda: enc.Encrypt(pt, ct), lambda: enc.addPtToCt(1, pt, ct), lambda: dec.Decrypt(ct, pt)):
            with pytest.raises(HeringError) as e:
                call()
            assert e.value.code == HE_EINVAL
    finally:
        g = C.c_uint64()
        assert load.he_graph_end(ctx.h, C.byref(g)) == 0
        load.he_graph_destroy(g.value)
    assert prng.Position() == pos


def test_launch_census(ctx):
    """the launches of a call do not depend on N, the level or the batch"""
    def census(c):
        rg = rig(ctx, c.logN, c.nq, c.npp)
        prng = sampling.PRNG(R.seeded_source(c.seed).read)
        enc = E.Encryptor(rg.ev, prng, device_key(rg, c), K.XS_P, K.SIGMA, K.BOUND)
        ct = element_for(rg, c, 1, 0)
        enc.EncryptZero(ct)
        ctx.sync()
        ctx.prof_begin()
        enc.EncryptZero(ct)
        ctx.sync()
        return sum(v[0] for v in ctx.prof_end().values())
    sk = [census(c) for c in K.ZERO_CASES[:3]]
    pk = [census(c) for c in K.ZERO_CASES[8:11]]
    print("launches: EncryptZero sk", sk, "pk", pk)
    assert len(set(sk)) == 1 and len(set(pk)) == 1
