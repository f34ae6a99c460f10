"""rgsw.Encryptor and blindrot.GenEvaluationKeyNew on the device (include/hering_rgsw_encryptor.h) against the restatement of the
reference (tests/rgsw_encryptor_ref.py): every word, and the position of the source afterwards.  The cases are those of
tests/rgsw_encryptor_cases.py, each of which has passed the host check that exp / log cannot change a word of it."""
import ctypes as C
import gc
import os
import types

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd import HeringError, sampling
from lattigo_amd import blindrot as B
from lattigo_amd import encryptor as E
from lattigo_amd import keygen as KG
from lattigo_amd import rgsw as G
from oracle import oracle as O
from tests import blindrot_ref as BR
from tests import keygen_cases as K
from tests import keygen_ref as KR
from tests import rgsw_encryptor_aliasing as A
from tests import rgsw_encryptor_cases as GC
from tests import rgsw_encryptor_ref as GR
from tests import sampler_ref as R
from tests.gpu_common import ctx  # noqa: F401

pytestmark = pytest.mark.gpu
HE_EINVAL, HE_EPRNG = -1, -6
CHUNK = "HERING_RGSW_CHUNK_KEYS"
_RIGS = {}


class Rig:
    def __init__(self, ctx, c: K.Case):
        self.N = c.N
        self.oQ, self.oP = K.rings(c)
        self.gQ = la.Ring(ctx, c.N, c.Q, conjugate_invariant=c.ci)
        self.gP = la.Ring(ctx, c.N, c.P, conjugate_invariant=c.ci) if c.P else None
        self.ev = G.Evaluator(self.gQ, self.gP)


@pytest.fixture(scope="module", autouse=True)
def release_rigs():
    os.environ.pop(CHUNK, None)
    yield
    os.environ.pop(CHUNK, None)
    _RIGS.clear()
    gc.collect()


def rig(ctx, c: K.Case) -> Rig:
    key = (c.logN, c.Q, c.P, c.ci)
    if key not in _RIGS:
        _RIGS[key] = Rig(ctx, c)
    return _RIGS[key]


def up(ring, words):
    """[limbs][N] words (or None) as one polynomial; [m][limbs][N]: m entries"""
    if ring is None or words is None:
        return None
    a = np.asarray(words, dtype=np.uint64)
    if a.ndim == 2:
        a = a[None]
    return la.Poly(ring, a.shape[1], a.shape[0]).upload(a)


def device_secret(rg: Rig, c: K.Case):
    q, p = K.secret(c)
    return E.SecretKey(up(rg.gQ, q), up(rg.gP, p))


def encryptor(rg: Rig, c: K.Case, seed, sk=None):
    prng = sampling.PRNG(R.seeded_source(seed).read)
    return G.Encryptor(rg.ev, prng, sk or device_secret(rg, c), GC.SIGMA, GC.BOUND), prng


def new_ct(rg: Rig, c: K.Case):
    return G.NewCiphertext(rg.ev, c.levelQ, c.levelP, c.pw2)


def words(ct):
    return np.stack([ct.Value[0].download(), ct.Value[1].download()])


def plain(rg: Rig, c: K.Case, form=(True, True)):
    return E.Plaintext(up(rg.gQ, GC.plaintext(c)), form[0], form[1])


# ---- 1. word for word, position for position ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GC.CASES, ids=lambda c: c.id)
def test_encrypt(ctx, c):
    rg = rig(ctx, c)
    want, _, pos = GC.want_encrypt(c)
    enc, prng = encryptor(rg, c, c.seed + 1000)
    ct = new_ct(rg, c)
    assert ct.Value[0].Shape()[:3] == (c.rows, c.levelQ + 1, c.levelP + 1)
    pt = plain(rg, c)
    enc.Encrypt(pt, ct)
    assert np.array_equal(words(ct), GR.image(want))
    assert prng.Position() == pos
    assert np.array_equal(pt.Value.download()[0], GC.plaintext(c))


@pytest.mark.parametrize("form", [(False, False), (True, False), (True, True)], ids=["coefficients", "ntt", "ntt-montgomery"])
def test_plaintext_forms(ctx, form):
    c = GC.FORMS_CASE
    rg = rig(ctx, c)
    want, _, pos = GC.want_encrypt(c, form)
    enc, prng = encryptor(rg, c, c.seed + 1000)
    ct = new_ct(rg, c)
    enc.Encrypt(plain(rg, c, form), ct)
    assert np.array_equal(words(ct), GR.image(want)) and prng.Position() == pos


def test_encrypt_zero_is_encrypt_with_no_plaintext(ctx):
    c = GC.ORDER_CASE
    rg = rig(ctx, c)
    want, _, pos = GC.want_zero(c)
    got = []
    for how in ("zero", "nil", "sel"):
        enc, prng = encryptor(rg, c, c.seed + 1000)
        ct = new_ct(rg, c)
        if how == "zero":
            enc.EncryptZero(ct)
        elif how == "nil":
            enc.Encrypt(None, ct)
        else:
            enc.EncryptTable(up(rg.gQ, GC.table_plaintexts(c, 2)), [-1], [ct])
        got.append(words(ct))
        assert prng.Position() == pos, how
    assert all(np.array_equal(g, GR.image(want)) for g in got)


def test_non_rgsw_operands_go_to_the_rlwe_encryptor(ctx):
    c = GC.ORDER_CASE
    rg = rig(ctx, c)
    sk = device_secret(rg, c)
    a, pa = encryptor(rg, c, 77, sk)
    ct = E.Element([rg.gQ.NewPoly(), rg.gQ.NewPoly()], True, True)
    a.EncryptZero(ct)
    pb = sampling.PRNG(R.seeded_source(77).read)
    ct2 = E.Element([rg.gQ.NewPoly(), rg.gQ.NewPoly()], True, True)
    E.Encryptor(rg.ev, pb, sk, K.XS_P, GC.SIGMA, GC.BOUND).EncryptZero(ct2)
    assert pa.Position() == pb.Position() > 0 and all(np.array_equal(x.download(), y.download()) for x, y in zip(ct.Value, ct2.Value))


# ---- 2. the table ----------------------------------------------------------------------------------------------------------------------
def run_table(rg, c, sel, m, chunk=None):
    if chunk is None:
        os.environ.pop(CHUNK, None)
    else:
        os.environ[CHUNK] = str(chunk)
    try:
        enc, prng = encryptor(rg, c, c.seed + 2000)
        cts = [new_ct(rg, c) for _ in sel]
        enc.EncryptTable(up(rg.gQ, GC.table_plaintexts(c, m)), sel, cts)
        return [words(ct) for ct in cts], prng.Position()
    finally:
        os.environ.pop(CHUNK, None)


def test_table(ctx):
    c, sel, m = GC.TABLE_CASE, GC.TABLE_SEL, GC.TABLE_M
    rg = rig(ctx, c)
    want, _, pos = GC.want_table(c, tuple(sel), m)
    got, gpos = run_table(rg, c, sel, m)
    assert gpos == pos
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, GR.image(w)), k
    # five single calls on a source seeded alike
    enc, prng = encryptor(rg, c, c.seed + 2000)
    pts = GC.table_plaintexts(c, m)
    for k, s in enumerate(sel):
        ct = new_ct(rg, c)
        enc.Encrypt(None if s < 0 else E.Plaintext(up(rg.gQ, pts[s]), True, True), ct)
        assert np.array_equal(words(ct), got[k]), k
    assert prng.Position() == pos
    # chunk boundaries change neither a word nor the position
    for chunk in (1, 2):
        again, apos = run_table(rg, c, sel, m, chunk)
        assert apos == pos and all(np.array_equal(a, g) for a, g in zip(again, got)), chunk
    # a table of one is the single call
    one, opos = run_table(rg, c, sel[:1], m)
    enc, prng = encryptor(rg, c, c.seed + 2000)
    ct = new_ct(rg, c)
    enc.Encrypt(E.Plaintext(up(rg.gQ, pts[sel[0]]), True, True), ct)
    assert np.array_equal(one[0], words(ct)) and np.array_equal(one[0], got[0]) and opos == prng.Position()


def test_table_on_the_rejecting_modulus(ctx):
    """the one-workgroup uniform re-parse inside a table moves every later row of the stream"""
    c, sel = K.C_REJECT, GC.REJECT_TABLE_SEL
    rg = rig(ctx, c)
    want, _, pos = GC.want_table(c, tuple(sel), 1)
    got, gpos = run_table(rg, c, sel, 1)
    assert gpos == pos and all(np.array_equal(g, GR.image(w)) for g, w in zip(got, want))


# ---- 3. fused against composed ---------------------------------------------------------------------------------------------------------
def composed(rg: Rig, c: K.Case, prng, sk, pt):
    """the same ciphertext from entries that were there before: Encryptor.EncryptZero (he_encrypt_zero_qp, batch 1) on each row of
    Value[0] and Value[1] in turn, then he_gadget_add_poly with two keys"""
    enc = E.Encryptor(rg.ev, prng, sk, K.XS_P, GC.SIGMA, GC.BOUND)
    rq, rp = rg.gQ.AtLevel(c.levelQ), (rg.gP.AtLevel(c.levelP) if c.levelP >= 0 else None)
    q = np.zeros((2, c.rows, 2, c.levelQ + 1, c.N), dtype=np.uint64)
    p = np.zeros((2, c.rows, 2, c.levelP + 1, c.N), dtype=np.uint64)
    for r in range(c.rows):
        for u in range(2):
            ct = E.ElementQP([(rq.NewPoly(), rp.NewPoly() if rp is not None else None) for _ in range(2)], True, True, c.levelQ, c.levelP)
            enc.EncryptZero(ct)
            for k in range(2):
                q[u, r, k] = ct.Value[k][0].download()[0]
                if rp is not None:
                    p[u, r, k] = ct.Value[k][1].download()[0]
    nj = KR.base_two_sizes(c.Q, c.levelQ, c.levelP, c.pw2) if c.pw2 else None
    keys = [rg.ev.NewEvaluationKey(q[u], p[u] if c.levelP >= 0 else None, c.pw2, nj) for u in range(2)]
    KG.AddPolyTimesGadgetVectorToGadgetCiphertext(pt, keys)
    return G.Ciphertext(*keys)


@pytest.mark.parametrize("c", GC.COMPOSED_CASES, ids=lambda c: c.id)
def test_fused_equals_composed(ctx, c):
    rg = rig(ctx, c)
    sk = device_secret(rg, c)
    pt = plain(rg, c)
    enc, prng = encryptor(rg, c, c.seed + 700, sk)
    fused = new_ct(rg, c)
    enc.Encrypt(pt, fused)
    prng2 = sampling.PRNG(R.seeded_source(c.seed + 700).read)
    other = composed(rg, c, prng2, sk, pt.Value)
    assert np.array_equal(words(fused), words(other))
    assert prng.Position() == prng2.Position() > 0


# ---- 4. the component order of Value[1] -----------------------------------------------------------------------------------------------
def test_value1_c0_is_of_the_c1_as_drawn(ctx):
    """a plaintext that is nonzero in every limb under a secret of uniform words: the c0 rows of Value[1] are those of an EncryptZero
    from the same stream -- a kernel that multiplies the secret into c1 after the gadget term was added fails here"""
    c = GC.ORDER_CASE
    rg = rig(ctx, c)
    rng = np.random.default_rng(c.seed)
    skq = np.stack([rng.integers(1, q, c.N, dtype=np.uint64) for q in c.Q])
    skp = np.stack([rng.integers(1, q, c.N, dtype=np.uint64) for q in c.P])
    sk = E.SecretKey(up(rg.gQ, skq), up(rg.gP, skp))
    pt = GC.plaintext(c)
    assert all(limb.all() for limb in pt)
    out = []
    for zero in (False, True):
        enc, prng = encryptor(rg, c, c.seed + 900, sk)
        ct = new_ct(rg, c)
        enc.Encrypt(None if zero else plain(rg, c), ct)
        out.append(words(ct))
    full, zero = out
    assert np.array_equal(full[1][:, 0], zero[1][:, 0])      # c0 of Value[1]
    assert np.array_equal(full[0][:, 1], zero[0][:, 1])      # c1 of Value[0]
    assert not np.array_equal(full[1][:, 1], zero[1][:, 1]) and not np.array_equal(full[0][:, 0], zero[0][:, 0])
    # and the restatement under that secret
    oenc = GR.Encryptor(rg.oQ, rg.oP, R.seeded_source(c.seed + 900), (skq, skp), GC.SIGMA, GC.BOUND)
    assert np.array_equal(full, GR.image(oenc.encrypt(pt, True, True, c.levelQ, c.levelP, c.pw2)))


# ---- 5. launches -------------------------------------------------------------------------------------------------------------------------
def census(ctx, c: K.Case, n, chunk=None):
    rg = rig(ctx, c)
    sel = (GC.TABLE_SEL * n)[:n]
    run_table(rg, c, sel, GC.TABLE_M, chunk)  # (once outside: the scratch has its size)
    ctx.sync()
    if chunk is not None:
        os.environ[CHUNK] = str(chunk)
    try:
        enc, prng = encryptor(rg, c, c.seed + 2000)
        cts = [new_ct(rg, c) for _ in sel]
        pts = up(rg.gQ, GC.table_plaintexts(c, GC.TABLE_M))
        ctx.sync()
        ctx.prof_begin()
        enc.EncryptTable(pts, sel, cts)
        ctx.sync()
        prof = ctx.prof_end()
    finally:
        os.environ.pop(CHUNK, None)
    return sum(v[0] for v in prof.values()), prof


def test_launch_census(ctx):
    """launches - 2 T - D with T = 2 n R table rows and D the per-key refreshes of the derived double-precision copy (none here: a
    base-2 key has none): the same for n = 1, 2 and 5 in one chunk, at most 7; with chunks forced to 1 it scales with the chunks.
    The composition of the earlier entries takes 10 T + 2 n."""
    c = GC.TABLE_CASE
    R_ = c.rows
    rest = {}
    for n in (1, 2, 5):
        total, prof = census(ctx, c, n)
        T = 2 * n * R_
        print(c.id, "n", n, "T", T, "launches", total, {k: v[0] for k, v in prof.items()})
        assert prof["rgsw_table_finish"][0] == 1 and prof["sampler_uniform"][0] == prof["sampler_gaussian"][0] == T
        assert "sampler_uniform_chain" not in prof  # (no rejected word)
        rest[n] = total - 2 * T
    assert len(set(rest.values())) == 1 and rest[1] <= 7, rest
    total, prof = census(ctx, c, 5, chunk=1)
    assert prof["rgsw_table_finish"][0] == 5 and total - 2 * (2 * 5 * R_) == 5 * rest[1]
    total, prof = census(ctx, c, 5, chunk=2)
    assert prof["rgsw_table_finish"][0] == 3 and total - 2 * (2 * 5 * R_) == 3 * rest[1]
    nop, prof = census(ctx, K.C_B16_NOP, 2)
    assert nop - 2 * (2 * 2 * K.C_B16_NOP.rows) == rest[1] - 1  # without special primes: no expansion on P


# ---- 6. refusals (host-side rejections only) ---------------------------------------------------------------------------------------------
def refused(call, code=HE_EINVAL):
    with pytest.raises(HeringError) as e:
        call()
    assert e.value.code == code, e.value


def test_refusals_touch_nothing(ctx):
    c = GC.TABLE_CASE
    rg = rig(ctx, c)
    sk = device_secret(rg, c)
    enc, prng = encryptor(rg, c, 1, sk)
    ct, ct2 = new_ct(rg, c), new_ct(rg, c)
    pt = plain(rg, c)
    pts = up(rg.gQ, GC.table_plaintexts(c, 2))
    # a public key bound, or no key
    kg = KG.KeyGenerator(rg.ev, sampling.PRNG(R.seeded_source(2).read), K.XS_P, GC.SIGMA, GC.BOUND)
    pk = kg.GenPublicKeyNew(sk)
    for key in (pk, None):
        e2 = G.Encryptor(rg.ev, prng, None, GC.SIGMA, GC.BOUND)
        e2._bind(key)
        for call in (lambda: e2.EncryptZero(ct), lambda: e2.Encrypt(pt, ct), lambda: e2.EncryptTable(pts, [0], [ct])):
            refused(call)
    # a bound key without the P part the ciphertext needs
    refused(lambda: G.Encryptor(rg.ev, prng, E.SecretKey(sk.Q, None), GC.SIGMA, GC.BOUND).EncryptZero(ct))
    # shapes of rgsw0 and rgsw1 that differ; keys of another evaluator; a shape genEvaluationKey does not serve
    low = G.NewCiphertext(rg.ev, c.levelQ - 1, c.levelP, c.pw2)
    L = la.load()
    assert L.he_rgsw_encrypt_zero(enc.h, ct.Value[0].h, low.Value[1].h) == HE_EINVAL
    refused(lambda: enc.EncryptTable(pts, [0, 1], [ct, low]))
    other = Rig(ctx, c)
    refused(lambda: enc.EncryptZero(new_ct(other, c)))
    # one key twice: within a ciphertext, across a table
    assert L.he_rgsw_encrypt_zero(enc.h, ct.Value[0].h, ct.Value[0].h) == HE_EINVAL
    refused(lambda: enc.EncryptTable(pts, [0, 1], [ct, ct]))
    refused(lambda: enc.EncryptTable(pts, [0, 1], [ct, G.Ciphertext(ct2.Value[0], ct.Value[1])]))
    assert sorted({n for n, _, _ in A.PAIRS}) == sorted(A.ROWS)
    # sel out of range, a plaintext table of too few limbs or of another ring, a batched single plaintext
    for sel in ([2, 0], [0, -2], [0, 1 << 20]):
        refused(lambda: enc.EncryptTable(pts, sel, [ct, ct2]))
    refused(lambda: enc.EncryptTable(None, [0, -1], [ct, ct2]))
    refused(lambda: enc.EncryptTable(up(rg.gQ, GC.table_plaintexts(c, 2)[:, :1]), [0, 1], [ct, ct2]))
    refused(lambda: enc.Encrypt(E.Plaintext(pts, True, True), ct))
    refused(lambda: enc.EncryptTable(pts, [], []))
    assert prng.Position() == 0 and not words(ct).any() and not words(ct2).any()


def test_refused_inside_a_graph_capture(ctx):
    c = GC.TABLE_CASE
    rg = rig(ctx, c)
    enc, prng = encryptor(rg, c, 3)
    ct = new_ct(rg, c)
    pt = plain(rg, c)
    enc.Encrypt(pt, ct)  # (once outside, as a capture asks)
    pos, img = prng.Position(), words(ct)
    L = la.load()
    assert L.he_graph_begin(ctx.h) == 0
    try:
        for call in (lambda: enc.EncryptZero(ct), lambda: enc.Encrypt(pt, ct), lambda: enc.EncryptTable(pt.Value, [0], [ct])):
            refused(call)
    finally:
        g = C.c_uint64()
        assert L.he_graph_end(ctx.h, C.byref(g)) == 0
        L.he_graph_destroy(g.value)
    assert prng.Position() == pos and np.array_equal(words(ct), img)


def test_a_source_that_fails_mid_table_stops_after_the_last_draw(ctx):
    c, sel, m = GC.TABLE_CASE, GC.TABLE_SEL, GC.TABLE_M
    rg = rig(ctx, c)
    oenc, osrc = GC.encryptor(c, c.seed + 2000)
    oenc.encrypt_table(GC.table_plaintexts(c, m), sel, c.levelQ, c.levelP, c.pw2)
    bounds = oenc.positions  # the position after every draw
    limit = bounds[len(bounds) // 2] + 100  # runs dry inside the third ciphertext
    src = R.seeded_source(c.seed + 2000)
    served = [0]

    def read(n):
        if served[0] + n > limit:
            return b""
        served[0] += n
        return src.read(n)
    prng = sampling.PRNG(read)
    enc = G.Encryptor(rg.ev, prng, device_secret(rg, c), GC.SIGMA, GC.BOUND)
    cts = [new_ct(rg, c) for _ in sel]
    refused(lambda: enc.EncryptTable(up(rg.gQ, GC.table_plaintexts(c, m)), sel, cts), HE_EPRNG)
    pos = prng.Position()
    # (a draw fetches at most 2048 bytes at this shape -- two 128-word uniform buffers, or the Gaussian's look-ahead -- so the draw
    # that failed began less than that before the limit)
    assert limit - 4096 < pos <= limit and pos in bounds
    # a source that fails at once: unchanged
    dry = sampling.PRNG(lambda n: b"")
    refused(lambda: G.Encryptor(rg.ev, dry, device_secret(rg, c), GC.SIGMA, GC.BOUND).EncryptZero(cts[0]), HE_EPRNG)
    assert dry.Position() == 0


# ---- 7. blindrot.GenEvaluationKeyNew, end to end -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blindrot_keys(ctx):
    """secret keys from the device KeyGenerator, the key set from seeded sources on the device"""
    c = GC.E2E_CASE
    rg = rig(ctx, c)
    gL = la.Ring(ctx, GC.N_LWE, [GC.Q_LWE])
    sk = KG.KeyGenerator(rg.ev, sampling.PRNG(R.seeded_source(c.seed + 5000).read), K.XS_P, GC.SIGMA, GC.BOUND).GenSecretKeyNew()
    skl = KG.KeyGenerator(la.Evaluator(gL, None), sampling.PRNG(R.seeded_source(c.seed + 7000).read), K.XS_P, GC.SIGMA, GC.BOUND).GenSecretKeyNew()
    assert np.array_equal(sk.Q.download()[0], K.secret(c)[0]) and np.array_equal(skl.Q.download()[0], GC.lwe_secret())
    prng, prng_kg = sampling.PRNG(R.seeded_source(c.seed + 3000).read), sampling.PRNG(R.seeded_source(c.seed + 3001).read)
    BRK = B.GenEvaluationKeyNew(rg.ev, sk, gL, skl, KG.EvaluationKeyParameters(c.levelQ, c.levelP, c.pw2), prng=prng, prngKeyGen=prng_kg,
                                XeSigma=GC.SIGMA, XeBound=GC.BOUND)
    return dict(rg=rg, gL=gL, sk=sk, skl=skl, BRK=BRK, pos=(prng.Position(), prng_kg.Position()))


def test_blind_rotation_keys_word_for_word(ctx, blindrot_keys):
    k = blindrot_keys
    brk, gks, _, pos = GC.want_blindrot(False)
    BRK = k["BRK"]
    assert len(BRK.BlindRotationKeys) == GC.N_LWE and list(BRK.AutomorphismKeys) == list(gks) == B.GaloisElements(GC.E2E_CASE.N)
    for i, (ct, w) in enumerate(zip(BRK.BlindRotationKeys, brk)):
        assert np.array_equal(words(ct), GR.image(w)), i
    for g, key in BRK.AutomorphismKeys.items():
        assert np.array_equal(key.download(), KR.image(gks[g])), g
    assert k["pos"] == pos
    assert np.array_equal(k["skl"].Q.download()[0], GC.lwe_secret())


def test_blind_rotation_keys_on_one_source(ctx, blindrot_keys):
    """the encryptor and the generator on one PRNG: all RGSW ciphertexts draw first, the Galois keys after them"""
    k = blindrot_keys
    c = GC.E2E_CASE
    brk, gks, _, (pos, _) = GC.want_blindrot(True)
    prng = sampling.PRNG(R.seeded_source(c.seed + 3000).read)
    BRK = B.GenEvaluationKeyNew(k["rg"].ev, k["sk"], k["gL"], k["skl"], KG.EvaluationKeyParameters(c.levelQ, c.levelP, c.pw2), prng=prng,
                                XeSigma=GC.SIGMA, XeBound=GC.BOUND)
    assert prng.Position() == pos
    assert all(np.array_equal(words(ct), GR.image(w)) for ct, w in zip(BRK.BlindRotationKeys, brk))
    assert all(np.array_equal(key.download(), KR.image(gks[g])) for g, key in BRK.AutomorphismKeys.items())


@pytest.mark.parametrize("ntt_flag", [True, False], ids=["NTTFlag", "coefficients"])
def test_evaluate_end_to_end(ctx, blindrot_keys, ntt_flag):
    """at the parameters of tests/test_gpu_blindrot.py::test_evaluate_end_to_end: Evaluate on the device with the generated key set
    equals the oracle's Evaluate over the downloaded key words, bit for bit, and decodes by that test's criterion"""
    k = blindrot_keys
    c = GC.E2E_CASE
    rg, BRK = k["rg"], k["BRK"]
    oev = O.Evaluator(rg.oQ, None)
    rL = GC.lwe_ring()
    nj = KR.base_two_sizes(c.Q, c.levelQ, c.levelP, c.pw2)

    def okey(key):
        w = key.download()
        return O.EvaluationKey(w[:, :, :c.levelQ + 1], w[:, :, c.levelQ + 1:], pw2=c.pw2, nj=nj)
    obrk = [[okey(ct.Value[0]), okey(ct.Value[1])] for ct in BRK.BlindRotationKeys]
    ogks = {g: okey(key) for g, key in BRK.AutomorphismKeys.items()}
    osk = types.SimpleNamespace(Q=K.secret(c)[0])
    oskl = types.SimpleNamespace(Q=GC.lwe_secret())
    slots = 8
    values = [-1 + 2 * i / slots for i in range(slots)]
    ct = BR.encrypt_lwe_values(np.random.default_rng(9800), rL, oskl, values, GC.Q_LWE / 4.0)
    scaleBR = GC.Q27 / 4.0
    otest = BR.init_test_polynomial(BR.sign, scaleBR, rg.oQ, -1, 1)
    want = BR.evaluate(oev, rL, ct, {i: otest for i in range(slots)}, obrk, ogks, ntt_flag)
    dtest = B.InitTestPolynomial(BR.sign, scaleBR, rg.gQ, -1, 1)
    ev = B.Evaluator(rg.ev, k["gL"], NTTFlag=ntt_flag)
    dct = [la.Poly(k["gL"], 1, 1).upload(ct[x][None]) for x in range(2)]
    res = ev.Evaluate(dct, {i: dtest for i in range(slots)}, BRK)
    assert sorted(res) == sorted(want)
    for i, v in enumerate(values):
        got = np.stack([p.download()[0] for p in res[i]])
        assert np.array_equal(got, want[i]), i
        if v != 0:
            a = BR.decode(rg.oQ, got, osk, scaleBR, is_ntt=ntt_flag)
            assert round(a * 8) / 8 == BR.sign(v), (i, v, a)


def test_blind_rotation_refusals(ctx, blindrot_keys):
    k = blindrot_keys
    c = GC.E2E_CASE
    rg = k["rg"]
    prng = sampling.PRNG(R.seeded_source(5).read)
    params = KG.EvaluationKeyParameters(c.levelQ, c.levelP, c.pw2)
    big = la.Ring(ctx, 2 * GC.N_LWE, [GC.Q_LWE])
    refused(lambda: B.GenEvaluationKeyNew(rg.ev, k["sk"], big, k["skl"], params, prng=prng))  # skLWE is not of ringLWE
    L = la.load()
    enc = G.Encryptor(rg.ev, prng, k["sk"], GC.SIGMA, GC.BOUND)
    kgen = KG.KeyGenerator(rg.ev, prng, K.XS_P, GC.SIGMA, GC.BOUND)
    cts = [new_ct(rg, c) for _ in range(GC.N_LWE)]
    gks = [kgen.NewEvaluationKey(params) for _ in range(11)]
    H = C.c_uint64
    a0, a1 = (H * GC.N_LWE)(*[x.Value[0].h for x in cts]), (H * GC.N_LWE)(*[x.Value[1].h for x in cts])
    call = lambda n, g: L.he_blindrot_gen_evaluation_key(enc.h, kgen.h, k["gL"].h, k["skl"].Q.h, n, a0, a1, (H * 11)(*g))
    assert call(GC.N_LWE - 1, [x.h for x in gks]) == HE_EINVAL                         # n is not the LWE degree
    assert call(GC.N_LWE, [gks[0].h] * 11) == HE_EINVAL                                 # one Galois key eleven times
    assert call(GC.N_LWE, [cts[0].Value[0].h] + [x.h for x in gks[1:]]) == HE_EINVAL    # a Galois key that is an RGSW key
    assert prng.Position() == 0 and not words(cts[0]).any()
