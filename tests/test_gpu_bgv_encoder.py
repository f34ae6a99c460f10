"""bgv.Encoder on the device (include/hering_bgv_encoder.h): every comparison is np.array_equal against the restatement of the
reference in tests/bgv_encoder_ref.py (held against definitions by tests/test_bgv_encoder_host.py).  Rings of logN 10 to 12 with
55-bit primes unless a case needs more (the two-pass transform at logN 13, the 32-limb cap of RingQ2T)."""
import gc
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd import _lib
from lattigo_amd import bgv
from tests import bfv_ref as F
from tests import bgv_encoder_ref as R
from tests.gpu_common import ctx  # noqa: F401
from tests.helpers import prod, rng_for, uniform_poly
from tests.rlwe_fixtures import SecretKey, downstream_primes, phase, small_to_rns

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T60 = downstream_primes(60, 1 << 14, 1)[0]  # a 60-bit plaintext modulus = 1 mod 2N for every N used here, above every q_i
_RIGS = {}


class Rig:
    """one parameter set on the device and in the restatement, with its encoder"""

    def __init__(self, ctx, logN, nq, T, npp=0):
        pr = downstream_primes(55, 2 << logN, nq + npp)
        self.P = R.Params(logN, pr[:nq], T, pr[nq:])
        self.N, self.NT, self.gap, self.T, self.q, self.p = self.P.N, self.P.NT, self.P.gap, T, self.P.q, self.P.p
        self.gQ = la.Ring(ctx, self.N, self.q)
        self.gP = la.Ring(ctx, self.N, self.p) if npp else None
        self.gT = la.Ring(ctx, self.NT, [T])
        self.enc = bgv.Encoder(self.gQ, self.gT, self.gP)


@pytest.fixture(scope="module", autouse=True)
def release_rigs():
    """the shared parameter sets are released with the module, while the library can still be reached: a device object that
    outlives the interpreter's shutdown is destroyed after the HIP runtime is"""
    yield
    _RIGS.clear()
    gc.collect()


def rig(ctx, logN, nq, T, npp=0):
    key = (logN, nq, T, npp)
    if key not in _RIGS:
        _RIGS[key] = Rig(ctx, logN, nq, T, npp)
    return _RIGS[key]


def eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


U64_EDGES = lambda T: np.array([0, 1, T - 1, T, T + 1, 1 << 63, (1 << 64) - 1], dtype=np.uint64)
I64_EDGES = lambda T: np.array([0, 1, -1, T - 1, -(T - 1), T, -T, T + 1, -(T + 1), -2 * T, (1 << 63) - 1, -(1 << 63)], dtype=np.int64)


def values_for(rng, T, n, signed):
    """n values: the edge words first, random ones after"""
    e = I64_EDGES(T) if signed else U64_EDGES(T)
    r = rng.integers(-(1 << 62), 1 << 62, n).astype(np.int64) if signed else rng.integers(0, 1 << 64, n, dtype=np.uint64)
    k = min(n, len(e))
    r[:k] = e[:k]
    return r


# ---- the index matrix ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,logNT", [(97, 4), (257, 7), (65537, 10)])
def test_index_matrix(ctx, T, logNT):
    rg = rig(ctx, 10, 2, T)
    assert (rg.enc.LogMaxSlots, rg.enc.LogGap, rg.enc.RingQ2TMaxLimbs) == (logNT, 10 - logNT, 32)
    assert eq(rg.enc.IndexMatrix(), R.permute_matrix(logNT))


# ---- EncodeRingT / DecodeRingT ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [97, 257, 65537, T60])
def test_encode_decode_ring_t(ctx, T):
    rg = rig(ctx, 10, 2, T)
    rng = rng_for(7000 + T % 1000)
    for scale in (1, T - 1, int(rng.integers(2, T - 1))):
        for n, batch, signed in itertools.product((1, rg.NT - 1, rg.NT), (1, 3), (False, True)):
            v = np.stack([values_for(rng, T, n, signed) for _ in range(batch)])
            pT = la.Poly(rg.gT, 1, batch, zero=False)
            rg.enc.EncodeRingT(v if batch > 1 else v[0], scale, pT)
            got = pT.download()
            for b in range(batch):
                assert eq(got[b], rg.P.encode_ring_t(v[b], scale, signed)), (scale, n, batch, signed, b)
            # decode what was encoded, and random words of ringT
            for words in (got, rng.integers(0, T, (batch, 1, rg.NT), dtype=np.uint64)):
                pT.upload(words)
                for out_signed in (False, True):
                    d = rg.enc.DecodeRingT(pT, scale, signed=out_signed)
                    for b in range(batch):
                        assert eq(d[b], rg.P.decode_ring_t(words[b], scale, out_signed)), (scale, n, batch, out_signed, b)
                assert eq(pT.download(), words)  # the input is not changed
            back = rg.enc.DecodeRingT(pT.upload(got), scale, signed=signed)
            want = np.array([[x % T for x in map(int, row)] for row in v], dtype=object)
            assert np.array_equal(np.array([[int(x) % T for x in row[:n]] for row in back], dtype=object), want)


# ---- RingT2Q ---------------------------------------------------------------------------------------------------------------------
def poison_case():
    """run by test_outputs_are_written_in_full in a process of its own with HERING_POISON=1: the outputs are scratch polynomials,
    so the zeros between and after the strides are the kernels' own stores"""
    c = la.Context(0)
    rng = rng_for(7100)
    for T in (97, 257, 65537, T60):
        rg = Rig(c, 10, 3, T, npp=2)
        for batch in (1, 3):
            words = rng.integers(0, T, (batch, 1, rg.NT), dtype=np.uint64)
            pT = la.Poly(rg.gT, 1, batch).upload(words)
            for scale_up, to_p in itertools.product((False, True), (False, True)):
                ring, top = (rg.gP, 1) if to_p else (rg.gQ, 2)
                for level in sorted({0, 1, top}):
                    out = la.Poly(ring, level + 1, batch, zero=False)
                    rg.enc.RingT2Q(level, scale_up, pT, out, to_p=to_p)
                    got = out.download()
                    for b in range(batch):
                        assert eq(got[b], rg.P.ring_t2q(words[b], level, scale_up, to_p)), (T, batch, scale_up, to_p, level, b)
            v = rng.integers(0, 1 << 64, (batch, max(rg.NT - 3, 1)), dtype=np.uint64)
            pq, pp, pt = la.Poly(rg.gQ, 3, batch, zero=False), la.Poly(rg.gP, 2, batch, zero=False), la.Poly(rg.gT, 1, batch, zero=False)
            rg.enc.EncodeQP(v, pq, pp, Scale=5, IsNTT=False, IsMontgomery=False)
            rg.enc.EncodeRingT(v, 5, pt)
            for b in range(batch):
                assert eq(pq.download()[b], rg.P.embed(v[b], 5, 2, False, False, False, False)), (T, b)
                assert eq(pp.download()[b], rg.P.embed(v[b], 5, 1, False, False, False, False, to_p=True)), (T, b)
                assert eq(pt.download()[b], rg.P.encode_ring_t(v[b], 5, False)), (T, b)
    print("poison OK")


def test_outputs_are_written_in_full(ctx):
    env = dict(os.environ, HERING_POISON="1")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c",
                        "import tests.conftest; from tests.test_gpu_bgv_encoder import poison_case; poison_case()"],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "poison OK" in r.stdout


def test_ring_t2q_takes_any_word(ctx):
    """words of pT at and above every q_i (T > q_i) and arbitrary 64-bit words: the Montgomery product takes them all"""
    rg = rig(ctx, 10, 2, T60)
    rng = rng_for(7150)
    words = rng.integers(0, 1 << 64, (1, 1, rg.NT), dtype=np.uint64)
    words[0, 0, :6] = [T60 - 1, rg.q[0], rg.q[0] - 1, rg.q[1] + 1, (1 << 64) - 1, 1 << 63]
    pT, out = la.Poly(rg.gT, 1).upload(words), la.Poly(rg.gQ, 2, zero=False)
    for scale_up in (False, True):
        rg.enc.RingT2Q(1, scale_up, pT, out)
        assert eq(out.get(), rg.P.ring_t2q(words[0], 1, scale_up)), scale_up


# ---- RingQ2T: the four branches --------------------------------------------------------------------------------------------------
def q2t_words(rng, rg, level):
    """[level + 1][N]: random words; on the coefficients RingQ2T reads, the edge list at every position of a wave; then words
    that put the float sum of the reconstruction within an ulp of an integer (tests/bfv_ref.py's construction)"""
    mods = rg.q[: level + 1]
    Q, T = prod(mods), rg.T
    w = uniform_poly(rng, mods, rg.N)
    edges = [0, 1, Q - 1, Q >> 1, (Q >> 1) + 1, (Q >> 1) - 1, T % Q, (Q - T) % Q]
    j = 0
    for j in range(min(512, rg.NT)):
        w[:, j * rg.gap] = R.words_of(edges[(j // 64 + j) % 8], mods)
    if level > 0:
        mu = F.ModUp(mods, [T])
        pats = [[q - 1 for q in mods], [1] * len(mods)] + [[q - 1 if k == i else 0 for k, q in enumerate(mods)] for i in range(len(mods))]
        pats += [[mods[0] - 1, 1] + [0] * (len(mods) - 2), [1, mods[1] - 1] + [0] * (len(mods) - 2)]
        for k, ys in enumerate(pats):
            if j + 1 + k < rg.NT:
                w[:, (j + 1 + k) * rg.gap] = mu.words_for_y(ys)
    return w


@pytest.mark.parametrize("T,logN", [(65537, 10), (T60, 10), (12289, 12), (257, 10), (97, 10)])
def test_ring_q2t(ctx, T, logN):
    rg = rig(ctx, logN, 4, T)
    rng = rng_for(7200 + T % 1000)
    for level, scale_down in itertools.product((0, 1, 3), (False, True)):
        w = q2t_words(rng, rg, level)
        pQ, pT = la.Poly(rg.gQ, level + 1).upload(w), la.Poly(rg.gT, 1, zero=False)
        rg.enc.RingQ2T(level, scale_down, pQ, pT)
        assert eq(pT.get(), rg.P.ring_q2t(w, level, scale_down)), (level, scale_down)
        assert eq(pQ.get(), w)


@pytest.mark.parametrize("T", [65537, 257])
def test_ring_q2t_32_limbs_and_the_cap(ctx, T):
    rg = rig(ctx, 10, 33, T)
    rng = rng_for(7300 + T % 1000)
    w = q2t_words(rng, rg, 31)
    pQ, pT = la.Poly(rg.gQ, 33).upload(np.concatenate([w, np.zeros((1, rg.N), dtype=np.uint64)])), la.Poly(rg.gT, 1, zero=False)
    for scale_down in (False, True):
        rg.enc.RingQ2T(31, scale_down, pQ, pT)
        assert eq(pT.get(), rg.P.ring_q2t(w, 31, scale_down)), scale_down
    before = pT.download()
    for call in (lambda: rg.enc.RingQ2T(32, False, pQ, pT), lambda: rg.enc.Decode(pQ, level=32)):
        with pytest.raises(la.HeringError) as err:
            call()
        assert err.value.code == -1 and eq(pT.download(), before)


def test_ring_roundtrip(ctx):
    """RingQ2T(RingT2Q(p)) == p, with and without scaling, gap 1 and gap 8"""
    for T in (65537, 257):
        rg = rig(ctx, 10, 4, T)
        words = rng_for(7350).integers(0, T, (2, 1, rg.NT), dtype=np.uint64)
        pT, pQ, back = la.Poly(rg.gT, 1, 2).upload(words), la.Poly(rg.gQ, 4, 2, zero=False), la.Poly(rg.gT, 1, 2, zero=False)
        for level, scaled in itertools.product((0, 3), (False, True)):
            rg.enc.RingT2Q(level, scaled, pT, pQ)
            rg.enc.RingQ2T(level, scaled, pQ, back)
            assert eq(back.download(), words), (T, level, scaled)


# ---- Encode / Embed / EncodeQP / Decode ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,logN", [(65537, 10), (257, 10), (97, 10), (T60, 11), (65537, 13)])
def test_encode_every_form(ctx, T, logN):
    rg = rig(ctx, logN, 3, T, npp=2)
    rng = rng_for(7400 + T % 1000 + logN)
    small = logN > 11  # (the restatement's transforms are the slow part: fewer combinations on the large ring)
    for batch in ((1,) if small else (1, 5)):
        for ntt, mont, scale_up in itertools.product((False, True), repeat=3):
            if small and not ntt:
                continue
            signed = bool(ntt ^ mont)
            n = rg.NT if scale_up else max(rg.NT - 5, 1)
            v = np.stack([values_for(rng, T, n, signed) for _ in range(batch)])
            scale = int(rng.integers(1, T))
            level = 2 if mont else 1
            pq = la.Poly(rg.gQ, 3, batch, zero=False)
            if scale_up:
                rg.enc.Encode(v, pq, Scale=scale, IsNTT=ntt, IsMontgomery=mont, level=level)
            else:
                rg.enc.Embed(v, pq, Scale=scale, IsNTT=ntt, IsMontgomery=mont, level=level)
            got = pq.download()
            for b in range(batch):
                assert eq(got[b, : level + 1], rg.P.embed(v[b], scale, level, ntt, mont, scale_up, signed)), (batch, ntt, mont, scale_up, b)
            for level_p in ((1,) if small else (-1, 0, 1)):
                pp = la.Poly(rg.gP, 2, batch, zero=False) if level_p >= 0 else None
                rg.enc.EncodeQP(v, pq, pp, Scale=scale, IsNTT=ntt, IsMontgomery=mont, levelQ=level, levelP=level_p, scaleUp=scale_up)
                got = pq.download()
                for b in range(batch):
                    assert eq(got[b, : level + 1], rg.P.embed(v[b], scale, level, ntt, mont, scale_up, signed)), (batch, ntt, mont, scale_up, b)
                    if pp is not None:
                        assert eq(pp.download()[b, : level_p + 1], rg.P.embed(v[b], scale, level_p, ntt, mont, scale_up, signed, to_p=True))


def test_encode_decode_coefficients(ctx):
    """IsBatched = false at N_T = N_Q; rejected when N_T < N_Q"""
    rg = rig(ctx, 10, 3, 65537, npp=2)
    rng = rng_for(7500)
    for signed, ntt, n in itertools.product((False, True), (False, True), (1, rg.N - 1, rg.N)):
        v = np.stack([values_for(rng, rg.T, n, signed) for _ in range(2)])
        pq = la.Poly(rg.gQ, 3, 2, zero=False)
        rg.enc.Encode(v, pq, Scale=7, IsBatched=False, IsNTT=ntt, IsMontgomery=True)  # (IsMontgomery is not read: no MForm)
        got = pq.download()
        d = rg.enc.Decode(pq, Scale=7, IsBatched=False, IsNTT=ntt, signed=signed)
        for b in range(2):
            assert eq(got[b], rg.P.encode_coeffs(v[b], 7, 2, ntt, signed)), (signed, ntt, n, b)
            assert eq(d[b], rg.P.decode(got[b], 7, 2, False, ntt, signed)), (signed, ntt, n, b)
    sp = rig(ctx, 10, 2, 257)
    pt = la.Poly(sp.gQ, 2)
    for call in (lambda: sp.enc.Encode(np.ones(4, dtype=np.uint64), pt, IsBatched=False), lambda: sp.enc.Decode(pt, IsBatched=False)):
        with pytest.raises(la.HeringError) as err:
            call()
        assert err.value.code == -1 and "N_T = N_Q" in str(err.value)


@pytest.mark.parametrize("T,logN", [(65537, 10), (T60, 10), (12289, 12), (97, 10)])
def test_decode(ctx, T, logN):
    rg = rig(ctx, logN, 4, T)
    rng = rng_for(7600 + T % 1000)
    for level, ntt, signed in itertools.product((0, 3), (False, True), (False, True)):
        w = np.stack([q2t_words(rng, rg, level) for _ in range(2)])
        pt = la.Poly(rg.gQ, level + 1, 2).upload(w)
        scale = int(rng.integers(1, T))
        d = rg.enc.Decode(pt, Scale=scale, IsNTT=ntt, signed=signed)
        for b in range(2):
            assert eq(d[b], rg.P.decode(w[b], scale, level, True, ntt, signed)), (level, ntt, signed, b)
        assert eq(pt.download(), w)


@pytest.mark.parametrize("T", [65537, 257])
def test_roundtrip_and_product_on_the_device(ctx, T):
    """Decode(Encode(v)) == v; Decode(Encode(a) * Embed(b)) == a o b mod T at the scale s^2 (one factor T^-1 in the product)"""
    rg = rig(ctx, 10, 3, T, npp=2)
    rng = rng_for(7700 + T % 1000)
    a, b = rng.integers(0, T, (2, rg.NT), dtype=np.uint64)
    s = int(rng.integers(2, T))
    pa, pb, pc = la.Poly(rg.gQ, 3, zero=False), la.Poly(rg.gQ, 3, zero=False), la.Poly(rg.gQ, 3, zero=False)
    rg.enc.Encode(a, pa, Scale=s, IsMontgomery=True)
    rg.gQ.unop("IMForm", pa, pc)
    assert eq(rg.enc.Decode(pc, Scale=s)[0], a)
    sa = a.astype(np.int64) - (T >> 1) - 1  # the centred range of :363 is [-(T >> 1) - 1, (T >> 1) - 1]
    rg.enc.Encode(sa, pc, Scale=s)
    assert eq(rg.enc.Decode(pc, Scale=s, signed=True)[0], sa)
    rg.enc.Embed(b, pb, Scale=s)
    rg.gQ.binop("MulCoeffsMontgomery", pa, pb, pc)
    want = np.array([int(x) * int(y) % T for x, y in zip(a, b)], dtype=np.uint64)
    assert eq(rg.enc.Decode(pc, Scale=s * s % T)[0], want)


def test_end_to_end_with_bgv_mul_relin(ctx):
    """encode on the device, encrypt on the host over the downloaded plaintexts, he_bgv_mul_relin, decrypt on the host, decode on the
    device: the slot-wise product"""
    T = 65537
    rg = rig(ctx, 10, 3, T, npp=2)
    rng = rng_for(7800)
    oQ = rg.P.oQ
    sk = SecretKey(rng, oQ, rg.P.oP)
    a, b = rng.integers(0, T, (2, rg.NT), dtype=np.uint64)
    cts = []
    for v in (a, b):
        pt = rg.enc.Encode(v, la.Poly(rg.gQ, 3, zero=False)).get()
        e = oQ.NTT(small_to_rns(np.clip(np.rint(rng.normal(0.0, 3.2, rg.N)), -19, 19).astype(np.int64), rg.q))
        c1 = uniform_poly(rng, rg.q, rg.N)
        c0 = oQ.binop("Sub", oQ.binop("Add", pt, e), oQ.binop("MulCoeffsMontgomery", c1, sk.Q))
        cts.append([rg.gQ.NewPoly().upload(c0), rg.gQ.NewPoly().upload(c1)])
    gev = la.Evaluator(rg.gQ, rg.gP)
    out = [rg.gQ.NewPoly() for _ in range(3)]
    gev.BGVMulRelin(2, T, cts[0], cts[1], None, out)
    ph = phase(oQ, np.stack([o.get() for o in out]), sk.Q)
    got = rg.enc.Decode(rg.gQ.NewPoly().upload(ph))[0]
    assert eq(got, np.array([int(x) * int(y) % T for x, y in zip(a, b)], dtype=np.uint64))


# ---- launches, rejections, scheduling --------------------------------------------------------------------------------------------
def census(ctx, call):
    ctx.sync()
    ctx.prof_begin()
    call()
    ctx.sync()
    return {k: v[0] for k, v in ctx.prof_end().items()}


def merged(*cs):
    out = {}
    for c in cs:
        for k, v in c.items():
            out[k] = out.get(k, 0) + v
    return out


@pytest.mark.parametrize("T,logN", [(65537, 10), (257, 10), (65537, 13)])
def test_launch_census(ctx, T, logN):
    """a batched NTT encode: the scatter and the fan-out, plus what the existing transforms launch for ringT (inverse) and ringQ
    (forward); EncodeQP adds the forward transform of P only; a decode: the inverse transform, one RNS -> T launch, the forward
    transform of ringT, the gather.  Whatever the level, the batch and the number of values."""
    rg = rig(ctx, logN, 3, T, npp=2)
    rng = rng_for(7900)
    seen = []
    for level, batch, n in ((0, 1, 1), (2, 3, rg.NT)):
        v = rng.integers(0, T, (batch, n), dtype=np.uint64)
        pq, pp, pT = la.Poly(rg.gQ, level + 1, batch), la.Poly(rg.gP, 2, batch), la.Poly(rg.gT, 1, batch)
        rq = rg.gQ.AtLevel(level)
        ntt_q, intt_q = census(ctx, lambda: rq.NTT(pq, pq)), census(ctx, lambda: rq.INTT(pq, pq))
        ntt_p = census(ctx, lambda: rg.gP.NTT(pp, pp))
        ntt_t, intt_t = census(ctx, lambda: rg.gT.NTT(pT, pT)), census(ctx, lambda: rg.gT.INTT(pT, pT))
        new = {"bgv_slots_to_t": 1, "bgv_t_to_rns": 1}
        c = census(ctx, lambda: rg.enc.Encode(v, pq, Scale=3, IsMontgomery=True))
        assert c == merged(new, intt_t, ntt_q), (c, intt_t, ntt_q)
        cqp = census(ctx, lambda: rg.enc.EncodeQP(v, pq, pp, Scale=3))
        assert cqp == merged(c, ntt_p), (cqp, c, ntt_p)
        assert census(ctx, lambda: rg.enc.Encode(v, pq, IsNTT=False)) == merged(new, intt_t)
        d = census(ctx, lambda: rg.enc.Decode(pq, Scale=3))
        assert d == merged({"bgv_rns_to_t": 1, "bgv_t_to_slots": 1}, intt_q, ntt_t), (d, intt_q, ntt_t)
        assert census(ctx, lambda: rg.enc.RingT2Q(level, True, pT, pq)) == {"bgv_t_to_rns": 1}
        assert census(ctx, lambda: rg.enc.RingQ2T(level, True, pq, pT)) == {"bgv_rns_to_t": 1}
        assert census(ctx, lambda: rg.enc.EncodeRingT(v, 3, pT)) == merged({"bgv_slots_to_t": 1, "ew": 1}, intt_t)
        assert census(ctx, lambda: rg.enc.DecodeRingT(pT, 3)) == merged({"bgv_t_to_slots": 1, "ew": 1}, ntt_t)
        seen.append((sum(c.values()), sum(cqp.values()), sum(d.values())))
    assert seen[0] == seen[1], seen  # independent of level, batch and n_values
    if logN == 13:
        assert sum(ntt_q.values()) == 2  # the two-pass route of the forward transform


def test_rejections_leave_every_operand_unchanged(ctx):
    T = 65537
    rg = rig(ctx, 10, 3, T, npp=2)
    other = rig(ctx, 11, 3, T60, npp=2)
    rng = rng_for(8000)
    pq = la.Poly(rg.gQ, 2).upload(uniform_poly(rng, rg.q[:2], rg.N))
    pp = la.Poly(rg.gP, 1).upload(uniform_poly(rng, rg.p[:1], rg.N))
    pT = la.Poly(rg.gT, 1).upload(rng.integers(0, T, (1, rg.NT), dtype=np.uint64))
    before = [x.download() for x in (pq, pp, pT)]
    e, v = rg.enc, rng.integers(0, T, rg.NT, dtype=np.uint64)
    no_p = bgv.Encoder(rg.gQ, rg.gT)
    L = _lib.load()
    raw = lambda fn, *a: _lib.check(fn(*a))
    vp = v.ctypes.data_as(_lib.u64p)
    out = np.zeros(rg.NT, dtype=np.uint64).ctypes.data_as(_lib.u64p)
    ctx2 = la.Context(0)
    ring2, ring2t = la.Ring(ctx2, rg.N, rg.q), la.Ring(ctx2, rg.NT, [T])
    foreign, foreign_t = ring2.NewPoly(), ring2t.NewPoly()
    sp = rig(ctx, 10, 2, 257)
    many = la.Poly(sp.gT, 1, 65536)
    calls = [
        lambda: e.Encode(v, pq, level=3), lambda: e.Encode(v, pq, level=-1),               # a level the ring lacks
        lambda: e.Encode(v, pq, level=2),                                                 # too few limbs
        lambda: e.EncodeQP(v, pq, pp, levelP=2), lambda: e.EncodeQP(v, pq, pp, levelP=1),
        lambda: e.Decode(pq, level=3), lambda: e.Decode(pq, level=2),
        lambda: e.RingT2Q(3, True, pT, pq), lambda: e.RingT2Q(2, True, pT, pq), lambda: e.RingT2Q(2, True, pT, pp, to_p=True),
        lambda: e.RingQ2T(3, True, pq, pT), lambda: e.RingQ2T(2, True, pq, pT),
        lambda: e.Encode(np.zeros(0, dtype=np.uint64), pq), lambda: e.EncodeRingT(np.zeros(0, dtype=np.uint64), 1, pT),   # n_values = 0
        lambda: e.Encode(np.zeros(rg.NT + 1, dtype=np.uint64), pq),                       # above slots
        lambda: e.Encode(np.zeros(rg.N + 1, dtype=np.uint64), pq, IsBatched=False),       # above N
        lambda: e.EncodeRingT(np.zeros(rg.NT + 1, dtype=np.uint64), 1, pT),
        lambda: raw(L.he_bgv_encode, e.h, 1, 1, 1, 1, 0, 1, None, 4, 0, 1, pq.h),         # values NULL
        lambda: raw(L.he_bgv_encode_qp, e.h, 1, 0, 1, 1, 0, 1, None, 4, 0, 1, pq.h, pp.h),
        lambda: raw(L.he_bgv_encode_ring_t, e.h, 1, None, 4, 0, 1, pT.h),
        lambda: raw(L.he_bgv_decode, e.h, 1, 1, 1, 1, pq.h, 0, None),
        lambda: raw(L.he_bgv_decode_ring_t, e.h, 1, pT.h, 0, None),
        lambda: raw(L.he_bgv_encode, e.h, 1, 1, 1, 1, 0, 1, vp, 4, 0, 0, pq.h),           # batch 0
        lambda: e.Encode(np.zeros((65536, 1), dtype=np.uint64), pq),                      # batch above 65535
        lambda: e.Encode(np.stack([v, v]), pq), lambda: e.EncodeRingT(np.stack([v, v]), 1, pT),   # not the polynomial's batch
        lambda: sp.enc.DecodeRingT(many, 1),                                                  # more than 65535 entries
        lambda: e.Encode(v, pq, Scale=0), lambda: e.Encode(v, pq, Scale=T), lambda: e.Decode(pq, Scale=0), lambda: e.Decode(pq, Scale=T + 1),
        lambda: e.EncodeRingT(v, 0, pT), lambda: e.DecodeRingT(pT, T),                    # scale outside [1, T)
        lambda: e.Encode(v, foreign), lambda: e.Decode(foreign), lambda: e.RingQ2T(1, True, pq, foreign_t),   # another context
        lambda: e.RingT2Q(1, True, foreign_t, pq), lambda: e.EncodeRingT(v, 1, foreign_t),
        lambda: e.Encode(v, la.Poly(other.gQ, 2)), lambda: e.Decode(la.Poly(other.gQ, 2)),  # another degree
        lambda: e.RingT2Q(1, True, la.Poly(other.gT, 1), pq), lambda: e.RingQ2T(1, True, pq, la.Poly(other.gT, 1)),
        lambda: e.EncodeQP(v, pq, pq, levelP=0),                                          # outP is outQ
        lambda: no_p.EncodeQP(v, pq, pp, levelP=0), lambda: no_p.RingT2Q(0, True, pT, pp, to_p=True),   # no ringP
    ]
    for i, call in enumerate(calls):
        with pytest.raises(la.HeringError) as err:
            call()
        assert err.value.code == -1, (i, str(err.value))
        assert all(eq(x.download(), w) for x, w in zip((pq, pp, pT), before)), i
    # encoder creation: the ring-T rule, one modulus, T coprime to Q and P, one context
    for bad in (lambda: bgv.Encoder(rg.gQ, la.Ring(ctx, 512, [T])),                      # logN_T below min(logN_Q, v2(T - 1) - 1)
                lambda: bgv.Encoder(rg.gQ, la.Ring(ctx, rg.N, [T, 12289])),              # two moduli
                lambda: bgv.Encoder(rg.gQ, la.Ring(ctx, rg.N, [rg.q[1]])),               # T = q_1
                lambda: bgv.Encoder(rg.gQ, la.Ring(ctx, rg.N, [rg.p[0]]), rg.gP),        # T = p_0
                lambda: bgv.Encoder(rg.gQ, ring2t),                                       # another context
                lambda: bgv.Encoder(rg.gQ, rg.gT, other.gP),                              # ringP of another degree
                lambda: bgv.Encoder(la.Ring(ctx, rg.N, [x for x in downstream_primes(55, 4 * rg.N, 2)], conjugate_invariant=True), rg.gT)):
        with pytest.raises(la.HeringError) as err:
            bad()
        assert err.value.code == -1, str(err.value)
    x, y = rg.gQ.NewPoly(), rg.gQ.NewPoly()
    rg.gQ.NTT(x, y)
    ctx.sync()
    with ctx.capture():
        rg.gQ.NTT(x, y)
        for call in (lambda: e.Encode(v, pq), lambda: e.Decode(pq), lambda: e.RingT2Q(1, True, pT, pq), lambda: e.RingQ2T(1, True, pq, pT),
                     lambda: e.EncodeRingT(v, 1, pT), lambda: e.DecodeRingT(pT, 1)):
            with pytest.raises(la.HeringError):
                call()  # host transfers cannot be captured
    assert all(eq(x.download(), w) for x, w in zip((pq, pp, pT), before))
    e.Encode(v, pq)
    assert eq(pq.get(), rg.P.embed(v, 1, 1, True, False, True, False))


@pytest.mark.parametrize("deferred", [0, 4])
def test_order_with_the_submission_queue(ctx, deferred):
    """an encode runs after the queued writers of its output, a decode after those of its input (he_poly_upload's rule)"""
    rg = rig(ctx, 10, 3, 65537, npp=2)
    rng = rng_for(8100 + deferred)
    v = rng.integers(0, rg.T, rg.NT, dtype=np.uint64)
    x = la.Poly(rg.gQ, 3).upload(uniform_poly(rng, rg.q, rg.N))
    pt, tmp = la.Poly(rg.gQ, 3), la.Poly(rg.gQ, 3)
    want = rg.P.embed(v, 3, 2, True, False, True, False)
    ctx.SetCoalescing(64, 500)
    if deferred:
        ctx.SetDeferred(deferred)
    try:
        for _ in range(3):
            rg.gQ.NTT(x, pt)                                  # a queued writer of the encode's output
            rg.enc.Encode(v, pt, Scale=3)
            assert eq(pt.get(), want)
            rg.gQ.NTT(x, tmp)
            rg.gQ.INTT(pt, tmp)                               # a queued writer of the decode's input
            assert eq(rg.enc.Decode(tmp, Scale=3, IsNTT=False)[0], v)
    finally:
        if deferred:
            ctx.SetDeferred(0)
        ctx.SetCoalescing(0, 0)


def test_encode_inside_a_recorded_window_fails_trace_end(ctx):
    rg = rig(ctx, 10, 2, 257)
    pt, pT = la.Poly(rg.gQ, 2), la.Poly(rg.gT, 1)
    v = np.ones(4, dtype=np.uint64)
    _lib.trace_begin()
    try:
        rg.enc.Decode(pt)
        rg.enc.DecodeRingT(pT, 1)
        rg.enc.IndexMatrix()
        prog = _lib.trace_end()
        assert prog.size == 0
        _lib.trace_begin()
        rg.enc.Encode(v, pt)
        with pytest.raises(RuntimeError, match="he_bgv_encode"):
            _lib.trace_end()
    finally:
        if _lib._trace is not None:
            try:
                _lib.trace_end()
            except RuntimeError:
                pass
