"""The ring samplers on the device (include/hering_sampler.h) against the restatement of the reference (tests/sampler_ref.py, held
against definitions by tests/test_sampler_host.py): every word, and the position of the source afterwards.  The Gaussian streams
are those of tests/sampler_streams.py, each of which has passed the host check that exp / log cannot change a word of it."""
import gc

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd import HeringError, sampling
from oracle import oracle as O
from tests import sampler_ref as R
from tests import sampler_streams as S
from tests.conftest import Pi60, Qi60
from tests.gpu_common import ctx  # noqa: F401

pytestmark = pytest.mark.gpu
HE_EINVAL, HE_EPRNG = -1, -6
_RINGS = {}


def upstream_primes(bits, nth_root, n):
    """primes 2^bits + 1 + k nth_root, k >= 0: just above a power of two, where the mask accepts half of the words"""
    out, x = [], (1 << bits) + 1
    while len(out) < n:
        if O.IsPrime(x):
            out.append(x)
        x += nth_root
    return out


# just below 2^61: nothing is rejected (2^-40 per word); just above a power of two: every other word is
BELOW_Q, BELOW_P = Qi60[:4], Pi60[:2]
ABOVE_Q = [65537, 576460752303439873] + upstream_primes(40, 1 << 13, 2)  # the reference's known-answer prime 2^59 + 2^14 + 1
ABOVE_P = upstream_primes(50, 1 << 13, 2)


@pytest.fixture(scope="module", autouse=True)
def release_rings():
    yield
    _RINGS.clear()
    gc.collect()


def ring(ctx, logN, moduli):
    key = (logN, tuple(moduli))
    if key not in _RINGS:
        _RINGS[key] = la.Ring(ctx, 1 << logN, list(moduli))
    return _RINGS[key]


def device_prng(src: R.Source):
    return sampling.PRNG(src.read)


def words(pols):
    return np.array(pols, dtype=np.uint64)


def start_poly(rng, r, batch, add):
    """(the device polynomial, its words as the restatement takes them or None): random canonical words for ReadAndAdd"""
    pol = r.NewPoly(batch)
    if not add:
        return pol, [None] * batch
    init = np.stack([np.stack([rng.integers(0, q, r.N, dtype=np.uint64) for q in r.moduli]) for _ in range(batch)])
    pol.upload(init)
    return pol, [[[int(w) for w in limb] for limb in e] for e in init]


# ---- uniform -----------------------------------------------------------------------------------------------------------------
UNIFORM = [(4, 1, 0, 1, "below"), (4, 3, 0, 3, "above"), (5, 4, 1, 3, "below"), (8, 2, 1, 3, "below"), (8, 2, 2, 1, "above"),
           (10, 1, 1, 3, "above"), (12, 4, 2, 3, "below"), (12, 4, 0, 1, "above"), (12, 3, 2, 3, "above")]


@pytest.mark.parametrize("add", [0, 1])
@pytest.mark.parametrize("logN,nq,npp,batch,kind", UNIFORM)
def test_uniform(ctx, logN, nq, npp, batch, kind, add):
    mq, mp = (BELOW_Q, BELOW_P) if kind == "below" else (ABOVE_Q, ABOVE_P)
    rq, rp = ring(ctx, logN, mq[:nq]), ring(ctx, logN, mp[:npp]) if npp else None
    rng = np.random.default_rng(logN * 100 + nq)
    seed = 1000 + logN * 10 + nq + npp
    ref = R.seeded_source(seed)
    prng = device_prng(R.seeded_source(seed))
    N = 1 << logN
    polq, initq = start_poly(rng, rq, batch, add)
    if rp is None:
        want = [R.uniform_read(ref, N, rq.moduli, initq[b]) for b in range(batch)]
        s = sampling.UniformSampler(prng, rq)
        (s.ReadAndAdd if add else s.Read)(polq)
        assert np.array_equal(polq.download(), words(want))
    else:
        polp, initp = start_poly(rng, rp, batch, add)
        want = [R.uniform_read_qp(ref, N, rq.moduli, rp.moduli, None if not add else (initq[b], initp[b])) for b in range(batch)]
        s = sampling.UniformSampler(prng, rq, rp)
        (s.ReadAndAdd if add else s.Read)((polq, polp))
        assert np.array_equal(polq.download(), words([w[0] for w in want]))
        assert np.array_equal(polp.download(), words([w[1] for w in want]))
    assert prng.Position() == ref.pos
    if kind == "below":
        assert ref.pos == batch * (-(-nq * N // 128) + -(-npp * N // 128)) * 1024


def test_uniform_at_a_level_below_the_top(ctx):
    rq, rp = ring(ctx, 8, BELOW_Q), ring(ctx, 8, BELOW_P)
    ref, prng = R.seeded_source(31), device_prng(R.seeded_source(31))
    polq, polp = rq.NewPoly(2), rp.NewPoly(2)
    before = polq.download()
    sampling.UniformSampler(prng, rq, rp).AtLevel(1, 0).Read((polq, polp))
    want = [R.uniform_read_qp(ref, 256, rq.moduli[:2], rp.moduli[:1]) for _ in range(2)]
    assert np.array_equal(polq.download()[:, :2], words([w[0] for w in want])) and np.array_equal(polq.download()[:, 2:], before[:, 2:])
    assert np.array_equal(polp.download()[:, :1], words([w[1] for w in want]))
    assert prng.Position() == ref.pos


REJ, ACC = (1 << 64) - 1, 5  # a word every modulus below its mask rejects; a word every modulus accepts


def be(ws):
    return b"".join(int(w).to_bytes(8, "big") for w in ws)


def run_uniform_bytes(ctx, data, logN, moduli, batch=1):
    r = ring(ctx, logN, moduli)
    ref, prng = R.bytes_source(data), device_prng(R.bytes_source(data))
    want = [R.uniform_read(ref, 1 << logN, r.moduli) for _ in range(batch)]
    got = sampling.UniformSampler(prng, r).ReadNew(batch)
    assert np.array_equal(got.download(), words(want))
    assert prng.Position() == ref.pos
    return ref.pos


def test_uniform_rejections_across_a_block_and_a_limb(ctx):
    """N = 64, two limbs: limb 0 is 60 accepted words, 10 rejected, 4 accepted; then 136 rejected words, which lie on the boundary
    of the limbs and cross the end of the first 1024-byte buffer (word 128); then limb 1"""
    data = be([ACC] * 60 + [REJ] * 10 + [ACC + 1] * 4 + [REJ] * 136 + list(range(64)))
    assert run_uniform_bytes(ctx, data, 6, ABOVE_Q[:2]) == 3072


def test_uniform_last_word_of_a_block_fetches_no_more(ctx):
    """N = 64, two limbs, nothing rejected: the 128th word is the last of the first buffer, and no second buffer is fetched; with
    one rejection exactly one more is"""
    assert run_uniform_bytes(ctx, be(range(128)), 6, ABOVE_Q[:2]) == 1024
    assert run_uniform_bytes(ctx, be(list(range(100)) + [REJ] + list(range(27)) + [9]), 6, ABOVE_Q[:2]) == 2048
    assert run_uniform_bytes(ctx, be(range(128)), 6, ABOVE_Q[:2], batch=2) == 2048


# ---- Gaussian ----------------------------------------------------------------------------------------------------------------
GAUSSIAN = [("random-logN4", 1, 0, 0), ("random-logN8-b3", 2, 1, 1), ("random-logN10-b3", 3, 1, 0), ("random-logN12", 4, 1, 0),
            ("random-logN12-b3", 4, 0, 1), ("bound-is-sigma-logN8-b3", 2, 0, 0), ("crafted-logN8", 2, 0, 0), ("crafted-logN8", 1, 1, 1),
            ("crafted-logN6-b3", 3, 0, 1)]


@pytest.mark.parametrize("name,nq,mont,add", GAUSSIAN)
def test_gaussian(ctx, name, nq, mont, add):
    case = S.GAUSS[name]
    r = ring(ctx, case.logN, BELOW_Q[:nq])
    ref, prng = case.source(), device_prng(case.source())
    pol, init = start_poly(np.random.default_rng(nq), r, case.batch, add)
    want = [R.gaussian_read(ref, r.N, r.moduli, case.sigma, case.bound, bool(mont), init[b]) for b in range(case.batch)]
    s = sampling.GaussianSampler(prng, r, case.sigma, case.bound, bool(mont))
    (s.ReadAndAdd if add else s.Read)(pol)
    assert np.array_equal(pol.download(), words(want))
    assert prng.Position() == ref.pos and ref.pos % 1024 == 0


# ---- ternary -----------------------------------------------------------------------------------------------------------------
TERNARY = [(4, 1, 1, 0.5), (8, 2, 3, 0.5), (12, 4, 3, 0.5), (4, 1, 1, 2 / 3), (8, 2, 3, 2 / 3), (12, 4, 3, 2 / 3), (12, 3, 1, 2 / 3),
           (8, 1, 3, 0.25), (10, 2, 1, 0.25), (8, 1, 3, 0.9), (10, 2, 1, 0.9)]


def run_ternary(ctx, make, logN, nq, batch, P, mont, add, words_=None):
    r = ring(ctx, logN, BELOW_Q[:nq])
    ref, prng = make(), device_prng(make())
    pol, init = start_poly(np.random.default_rng(logN), r, batch, add)
    want = [R.ternary_read(ref, r.N, r.moduli, P, bool(mont), init[b], words=words_) for b in range(batch)]
    s = sampling.TernarySampler(prng, r, P, bool(mont), _words=words_)
    (s.ReadAndAdd if add else s.Read)(pol)
    assert np.array_equal(pol.download(), words(want))
    assert prng.Position() == ref.pos
    return ref.pos


@pytest.mark.parametrize("mont,add", [(0, 0), (1, 1)])
@pytest.mark.parametrize("logN,nq,batch,P", TERNARY)
def test_ternary(ctx, logN, nq, batch, P, mont, add):
    pos = run_ternary(ctx, lambda: R.seeded_source(2000 + logN + nq), logN, nq, batch, P, mont, add)
    assert pos == batch * ((1 << logN) // 4 if P == 0.5 else 1 << logN)


@pytest.mark.parametrize("batch", [1, 3])
def test_ternary_crafted_walks(ctx, batch):
    """a walk of 31 columns with signs from the next byte; walks that need a second N-byte buffer (host test: what each is for)"""
    run_ternary(ctx, lambda: S.cat_source(S.KY_LONG_WALK, 5), 4, 1, batch, 2 / 3, 0, 0)
    assert run_ternary(ctx, lambda: S.cat_source(S.KY_REFILL, 5), 4, 2, batch, 2 / 3, 1, 0) >= 32 * batch - 16


@pytest.mark.parametrize("logN,batch", [(4, 3), (8, 1), (10, 3)])
def test_ternary_restart_on_d_above_one(ctx, logN, batch):
    """the restart of :283-285, which no density reaches: over the matrix words of sampler_streams.KY_WORDS_RESTART"""
    run_ternary(ctx, lambda: R.seeded_source(21), logN, 2, batch, 0.5, 0, 0, words_=S.KY_WORDS_RESTART)


# ---- sequences ---------------------------------------------------------------------------------------------------------------
def test_a_sequence_of_calls_stays_in_step(ctx):
    """uniform QP, Gaussian (which fetches ahead), ternary, uniform again on ONE source: the bytes fetched ahead by one call are
    served to the next"""
    case = S.GAUSS["sequence-logN8-b3"]
    rq, rp = ring(ctx, 8, BELOW_Q[:2]), ring(ctx, 8, BELOW_P[:1])
    N = 256
    src = case.source()
    # the Gaussian stream of the case starts at offset 0 of its source: the sequence reads it first
    ref, prng = case.source(), device_prng(src)
    g = sampling.GaussianSampler(prng, rq, case.sigma, case.bound, True).ReadNew(3)
    want_g = [R.gaussian_read(ref, N, rq.moduli, case.sigma, case.bound, True) for _ in range(3)]
    assert prng.FetchedAhead() > 0 and prng.Position() == ref.pos
    u = sampling.UniformSampler(prng, rq, rp).ReadNew(3)
    want_u = [R.uniform_read_qp(ref, N, rq.moduli, rp.moduli) for _ in range(3)]
    assert prng.Position() == ref.pos
    t = sampling.TernarySampler(prng, rq, 2 / 3, True).ReadNew(3)
    want_t = [R.ternary_read(ref, N, rq.moduli, 2 / 3, True) for _ in range(3)]
    assert prng.Position() == ref.pos
    h = sampling.TernarySampler(prng, rq, 0.5, False).ReadNew(1)
    want_h = [R.ternary_read(ref, N, rq.moduli, 0.5, False)]
    assert prng.Position() == ref.pos
    assert np.array_equal(g.download(), words(want_g)) and np.array_equal(t.download(), words(want_t))
    assert np.array_equal(h.download(), words(want_h))
    assert np.array_equal(u[0].download(), words([w[0] for w in want_u])) and np.array_equal(u[1].download(), words([w[1] for w in want_u]))


def test_the_system_source(ctx):
    """getrandom(2): words below their moduli, positions that advance by the reference's consumption"""
    rq = ring(ctx, 8, BELOW_Q[:2])
    prng = sampling.PRNG()
    a = sampling.UniformSampler(prng, rq).ReadNew(2).download()
    b = sampling.UniformSampler(prng, rq).ReadNew(2).download()
    assert prng.Position() == 2 * 2 * 4096
    assert all((a[:, j] < q).all() and (b[:, j] < q).all() for j, q in enumerate(rq.moduli)) and not np.array_equal(a, b)
    e = sampling.GaussianSampler(prng, rq, 3.2, 19.2, False).ReadNew(1).download()[0]
    c = np.where(e[0] > rq.moduli[0] // 2, rq.moduli[0] - e[0], e[0] % rq.moduli[0]).astype(np.int64)
    assert c.max() <= 19 and c.max() > 3 and prng.Position() % 1024 == 0


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def code(excinfo):
    return excinfo.value.code


def test_refusals(ctx):
    r = ring(ctx, 6, ABOVE_Q[:2])
    pol = r.NewPoly()
    prng = device_prng(R.bytes_source(b"", 0xFF))
    with pytest.raises(HeringError, match="64 times") as e:  # every word is rejected: the call ends, with an error
        sampling.UniformSampler(prng, r).Read(pol)
    assert code(e) == HE_EPRNG and prng.Position() == 0
    with pytest.raises(HeringError, match="arbitrary-precision") as e:
        sampling.GaussianSampler(prng, r, 2.0 ** 54, 2.0 ** 70, False).Read(pol)
    assert code(e) == HE_EINVAL
    for sigma, bound in ((0.0, 1.0), (-1.0, 1.0), (float("nan"), 1.0), (3.2, -1.0), (3.2, float("inf")), (3.2, 2.0 ** 63)):
        with pytest.raises(HeringError) as e:
            sampling.GaussianSampler(prng, r, sigma, bound, False).Read(pol)
        assert code(e) == HE_EINVAL
    for P in (0.0, 1.0, -0.5, 1.5, float("nan")):
        with pytest.raises(HeringError) as e:
            sampling.TernarySampler(prng, r, P, False).Read(pol)
        assert code(e) == HE_EINVAL
    with pytest.raises(HeringError, match="column 55") as e:  # 0, 1, 0, then ones: columns 3 to 54 and one more
        sampling.TernarySampler(device_prng(R.bytes_source(bytes([0xFA]), 0xFF)), r, 0.5, False, _words=S.KY_WORDS_RESTART).Read(pol)
    assert code(e) == HE_EINVAL
    with pytest.raises(HeringError, match="64 times") as e:  # zeros: a restart at every bit, for ever
        sampling.TernarySampler(device_prng(R.bytes_source(b"", 0)), r, 0.5, False, _words=S.KY_WORDS_RESTART).Read(pol)
    assert code(e) == HE_EPRNG
    short = sampling.PRNG(lambda n: b"\0" * (n - 1))
    with pytest.raises(HeringError, match="ran short") as e:
        sampling.UniformSampler(short, r).Read(pol)
    assert code(e) == HE_EPRNG and short.Position() == 0
    big = ring(ctx, 6, BELOW_Q[:3])
    with pytest.raises(HeringError) as e:  # too few limbs
        sampling.UniformSampler(prng, big).Read(r.NewPoly())
    assert code(e) == HE_EINVAL
    p2 = ring(ctx, 6, BELOW_P[:2])
    with pytest.raises(HeringError) as e:  # unequal batches
        sampling.UniformSampler(prng, big, p2).Read((big.NewPoly(2), p2.NewPoly(1)))
    assert code(e) == HE_EINVAL
    same = big.NewPoly()
    with pytest.raises(HeringError, match="one polynomial") as e:
        sampling.UniformSampler(prng, big, ring(ctx, 6, BELOW_Q[:2])).Read((same, same))
    assert code(e) == HE_EINVAL


def test_refused_inside_a_capture(ctx):
    r = ring(ctx, 6, BELOW_Q[:2])
    pol, x, y = r.NewPoly(), r.NewPoly(), r.NewPoly()
    prng = device_prng(R.seeded_source(5))
    sampling.UniformSampler(prng, r).Read(pol)
    r.NTT(x, y)
    ctx.sync()
    before, pos = pol.download(), prng.Position()
    with ctx.capture():
        r.NTT(x, y)
        for read in (sampling.UniformSampler(prng, r).Read, sampling.GaussianSampler(prng, r, 3.2, 19.2, False).Read,
                     sampling.TernarySampler(prng, r, 2 / 3, False).ReadAndAdd):
            with pytest.raises(HeringError, match="captured") as e:
                read(pol)
            assert code(e) == HE_EINVAL
    assert np.array_equal(pol.download(), before) and prng.Position() == pos


# ---- launches ----------------------------------------------------------------------------------------------------------------
def census(ctx, call):
    ctx.prof_begin()
    call()
    return {k: v[0] for k, v in ctx.prof_end().items()}


def test_launch_census(ctx):
    """the launches of a sampler call do not depend on N, the level or the batch"""
    seen = {}
    for logN, nq, batch, gauss in ((8, 1, 1, "census-logN8"), (12, 4, 3, "census-logN12-b3")):
        r = ring(ctx, logN, BELOW_Q[:nq])
        pol = r.NewPoly(batch)
        prng = device_prng(R.seeded_source(77))
        case = S.GAUSS[gauss]
        got = {
            "uniform": census(ctx, lambda: sampling.UniformSampler(prng, r).Read(pol)),
            "uniform+": census(ctx, lambda: sampling.UniformSampler(prng, r).ReadAndAdd(pol)),
            "gaussian": census(ctx, lambda: sampling.GaussianSampler(device_prng(case.source()), r, case.sigma, case.bound, True).Read(pol)),
            "ternary": census(ctx, lambda: sampling.TernarySampler(prng, r, 2 / 3, True).ReadAndAdd(pol)),
            "half": census(ctx, lambda: sampling.TernarySampler(prng, r, 0.5, False).Read(pol)),
        }
        seen[logN] = got
    assert seen[8] == seen[12]
    assert seen[8] == {"uniform": {"sampler_uniform": 1}, "uniform+": {"sampler_uniform": 1, "ew": 1},
                       "gaussian": {"sampler_gaussian": 1, "sampler_expand": 1}, "ternary": {"sampler_ternary_ky": 1, "sampler_expand": 1},
                       "half": {"sampler_ternary_half": 1, "sampler_expand": 1}}
