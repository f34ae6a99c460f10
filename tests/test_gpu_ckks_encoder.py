"""ckks.Encoder on the device (include/hering_ckks_encoder.h): every comparison is np.array_equal against the restatement
(tests/ckks_encoder_ref.py) fed the table of roots read back from the encoder (he_ckks_encoder_roots), so the words do not depend
on which libm built that table.  Rings of logN <= 10 and 1-3 limbs unless a case needs more (the one-workgroup threshold of the
transform, the limb cap of decode)."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd import _lib
from lattigo_amd import ckks
from oracle import oracle as O
from tests import ckks_encoder_ref as R
from tests.gpu_common import ctx  # noqa: F401
from tests.helpers import rng_for
from tests.rlwe_fixtures import downstream_primes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Rig:
    """one ring (standard or conjugate-invariant) on the device and in the oracle, its encoder and the table it holds"""

    def __init__(self, ctx, logN, nq, ci=False, bits=55, npp=0, roots=None, moduli=None):
        self.ctx, self.logN, self.N, self.ci = ctx, logN, 1 << logN, ci
        self.M = (4 if ci else 2) << logN
        pr = moduli or downstream_primes(bits, 2 * self.M, nq + npp)
        self.q, self.p = pr[:nq], pr[nq:]
        self.gQ, self.oQ = la.Ring(ctx, self.N, self.q, conjugate_invariant=ci), O.Ring(self.N, self.q, ci)
        self.gP = self.oP = None
        if self.p:
            self.gP, self.oP = la.Ring(ctx, self.N, self.p, conjugate_invariant=ci), O.Ring(self.N, self.p, ci)
        self.enc = ckks.Encoder(self.gQ, self.gP, roots=roots)
        t = self.enc.Roots()
        self.rre, self.rim = t.real.copy(), t.imag.copy()
        self.max_log_slots = self.enc.LogMaxSlots

    def want_words(self, z, log_slots, scale, level, ntt, mont, side="q"):
        """the restated Embed of one vector: [level + 1][N]"""
        ring, mods = (self.oQ, self.q) if side == "q" else (self.oP, self.p)
        mods = mods[: level + 1]
        coeffs = R.embed_coeffs(z, log_slots, self.N, self.ci, self.M, self.rre, self.rim)
        w = R.quantise_poly(coeffs, scale, mods, self.N)
        return self.finish(w, ring, mods, ntt, mont)

    @staticmethod
    def finish(w, ring, mods, ntt, mont):
        """NTTSparseAndMontgomery on the quantiser's words: the oracle's strict transforms of their residues"""
        if ntt or mont:
            w = np.array([[int(x) % q for x in row] for row, q in zip(w, mods)], dtype=np.uint64)
        if ntt:
            w = ring.NTT(w, level=len(mods) - 1)
        if mont:
            w = ring.unop("MForm", w, level=len(mods) - 1)
        return w


def eq(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def check_fft(rg, logn, batch, seed):
    n = 1 << logn
    rng = rng_for(seed)
    v = rng.uniform(-4, 4, (batch, n)) + 1j * rng.uniform(-4, 4, (batch, n))
    f, i = rg.enc.FFT(v if batch > 1 else v[0], logn), rg.enc.IFFT(v if batch > 1 else v[0], logn)
    f, i = f.reshape(batch, n), i.reshape(batch, n)
    for b in range(batch):
        wr, wi = R.special_fft(v[b].real, v[b].imag, rg.M, rg.rre, rg.rim)
        assert eq(f[b].real, wr) and eq(f[b].imag, wi), ("fft", logn, b)
        wr, wi = R.special_ifft(v[b].real, v[b].imag, rg.M, rg.rre, rg.rim)
        assert eq(i[b].real, wr) and eq(i[b].imag, wi), ("ifft", logn, b)


# ---- FFT / IFFT ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [False, True])
def test_fft_every_size_of_a_small_ring(ctx, ci):
    rg = Rig(ctx, 6, 1, ci=ci)
    assert rg.max_log_slots == (6 if ci else 5)
    for logn in range(rg.max_log_slots + 1):
        for batch in (1, 3):
            check_fft(rg, logn, batch, 5000 + logn)


def test_fft_full_and_sparse_logn10(ctx):
    rg = Rig(ctx, 10, 1)
    for logn, batch in ((9, 1), (9, 3), (6, 3), (3, 1)):  # logGap = 0, 3, 6
        check_fft(rg, logn, batch, 5100 + logn)


def test_fft_on_both_sides_of_the_one_workgroup_threshold(ctx):
    """the largest n one workgroup takes and the smallest on the multi-pass route, each on a one-limb ring of just the degree it
    needs; the threshold is the library's"""
    th = Rig(ctx, 6, 1).enc.FFTOneWorkgroupMaxLogN
    assert 10 <= th <= 13  # n 16 B within the 160 KiB of LDS a workgroup may declare
    rg = Rig(ctx, th + 1, 1)
    assert rg.enc.FFTOneWorkgroupMaxLogN == th and rg.max_log_slots == th
    check_fft(rg, th, 3, 5200)
    rg = Rig(ctx, th + 2, 1)
    check_fft(rg, th + 1, 1, 5201)
    check_fft(rg, th + 1, 3, 5202)


def test_caller_supplied_roots_are_what_is_used(ctx):
    base = Rig(ctx, 6, 1)
    t = base.enc.Roots().copy()
    rng = rng_for(5300)
    t = (t.real * (1 + rng.integers(-4, 5, t.size) * 2.0 ** -40)) + 1j * (t.imag * (1 + rng.integers(-4, 5, t.size) * 2.0 ** -40))
    rg = Rig(ctx, 6, 1, roots=t)
    assert eq(rg.enc.Roots().real, t.real) and eq(rg.enc.Roots().imag, t.imag)
    check_fft(rg, 5, 3, 5301)
    v = rng.uniform(-4, 4, 32) + 1j * rng.uniform(-4, 4, 32)
    assert not eq(rg.enc.FFT(v, 5), base.enc.FFT(v, 5))
    # the built-in table is he_ckks_roots_host's
    h = ckks.roots_host(base.M)
    assert eq(h.real, base.rre) and eq(h.imag, base.rim)
    with pytest.raises(la.HeringError):
        bad = t.copy()
        bad[3] = complex(math.nan, 0)
        ckks.Encoder(base.gQ, None, roots=bad)


# ---- the quantiser ---------------------------------------------------------------------------------------------------------------
def edge_rig(ctx):
    N = 64
    mods = [downstream_primes(b, 4 * N, 1)[0] for b in (30, 45, 61)]
    rg = Rig(ctx, 6, 3, moduli=mods)
    by_scale = {}
    for q in mods:
        for value, scale in R.quantiser_cases(q):
            by_scale.setdefault(scale, []).append(value)
    return rg, by_scale


def test_quantiser_edge_list_coefficient_encode(ctx):
    """Float64ToFixedPointCRT through he_ckks_encode, not batched: the words of the coefficient domain, quirks included, and their
    strict NTT"""
    rg, by_scale = edge_rig(ctx)
    seen = set()
    for scale, vals in by_scale.items():
        for at in range(0, len(vals), rg.N):
            chunk = np.array(vals[at: at + rg.N])
            want = R.quantise_poly(chunk, scale, rg.q, rg.N)
            seen |= {("q" if int(w) == q else "above" if int(w) > q else "below") for row, q in zip(want, rg.q) for w in row}
            pt = rg.gQ.NewPoly()
            rg.enc.Encode(chunk, pt, Scale=scale, IsBatched=False, IsNTT=False)
            assert eq(pt.get(), want), (scale, at)
            rg.enc.Encode(chunk, pt, Scale=scale, IsBatched=False, IsNTT=True)
            assert eq(pt.get(), Rig.finish(want, rg.oQ, rg.q, True, False)), (scale, at)
    assert seen == {"q", "above", "below"}


@pytest.mark.parametrize("mont", [False, True])
@pytest.mark.parametrize("ntt", [False, True])
def test_quantiser_edge_list_through_the_fused_kernel(ctx, ntt, mont):
    """the same list through Embed with one slot (the transform of one value is that value): real part at coefficient 0, imaginary
    part at N / 2, one batch entry per pair of cases"""
    rg, by_scale = edge_rig(ctx)
    for scale, vals in by_scale.items():
        vals = vals + [0.0] * (len(vals) & 1)
        z = np.array(vals[0::2]) + 1j * np.array(vals[1::2])
        B = len(z)
        pt = la.Poly(rg.gQ, 3, B)
        rg.enc.Encode(z[:, None], pt, Scale=scale, LogSlots=0, IsNTT=ntt, IsMontgomery=mont)
        got = pt.download()
        for b in range(B):
            coeffs = np.zeros(rg.N)
            coeffs[0], coeffs[rg.N // 2] = z[b].real, z[b].imag
            want = Rig.finish(R.quantise_poly(coeffs, scale, rg.q, rg.N), rg.oQ, rg.q, ntt, mont)
            assert eq(got[b], want), (scale, b)


# ---- Encode ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", [False, True])
def test_encode_levels_slots_domains(ctx, ci):
    rg = Rig(ctx, 8, 3, ci=ci)
    rng = rng_for(5400 + ci)
    mx = rg.max_log_slots
    for level in (0, 1, 2):
        for log_slots in (0, 1, mx - 1, mx):
            slots = 1 << log_slots
            for cplx, nv in ((True, slots), (False, slots), (True, max(1, slots - 3))):
                z = rng.uniform(-1, 1, nv) + (1j * rng.uniform(-1, 1, nv) if cplx else 0)
                ntt, mont = bool((level + log_slots) & 1), bool(log_slots & 2)
                pt = la.Poly(rg.gQ, 3, 1)
                before = pt.download()
                rg.enc.Encode(z if cplx else z.real, pt, Scale=2.0 ** 45, LogSlots=log_slots, IsNTT=ntt, IsMontgomery=mont, level=level)
                want = rg.want_words(z, log_slots, 2.0 ** 45, level, ntt, mont)
                got = pt.download()[0]
                assert eq(got[: level + 1], want), (level, log_slots, cplx, nv)
                assert eq(got[level + 1:], before[0][level + 1:])  # the limbs above the level are not touched


@pytest.mark.parametrize("log_scale", [30, 45, 90])
def test_encode_scales(ctx, log_scale):
    """2^90 >= 2^64 / max |coeff|: the big-number path of the quantiser inside a full encode"""
    rg = Rig(ctx, 8, 2)
    rng = rng_for(5500 + log_scale)
    for log_slots in (rg.max_log_slots, 3):
        z = rng.uniform(-1, 1, 1 << log_slots) + 1j * rng.uniform(-1, 1, 1 << log_slots)
        if log_scale == 90:
            c = R.embed_coeffs(z, log_slots, rg.N, False, rg.M, rg.rre, rg.rim)
            assert np.max(np.abs(c)) * 2.0 ** log_scale >= 2.0 ** 64
        for ntt in (False, True):  # (sparse and coefficient domain: the polynomial in Y = X^gap, the header's documented form)
            pt = rg.gQ.NewPoly()
            rg.enc.Encode(z, pt, Scale=2.0 ** log_scale, LogSlots=log_slots, IsNTT=ntt)
            assert eq(pt.get(), rg.want_words(z, log_slots, 2.0 ** log_scale, 1, ntt, False)), (log_slots, ntt)


def test_encode_qp_and_batches(ctx):
    rg = Rig(ctx, 8, 2, npp=1)
    rng = rng_for(5600)
    ls = rg.max_log_slots - 1
    z = rng.uniform(-1, 1, (3, 1 << ls)) + 1j * rng.uniform(-1, 1, (3, 1 << ls))
    pq, pp = la.Poly(rg.gQ, 2, 3), la.Poly(rg.gP, 1, 3)
    rg.enc.EncodeQP(z, pq, pp, Scale=2.0 ** 40, LogSlots=ls)
    gq, gp = pq.download(), pp.download()
    for b in range(3):
        assert eq(gq[b], rg.want_words(z[b], ls, 2.0 ** 40, 1, True, True, "q")), b
        assert eq(gp[b], rg.want_words(z[b], ls, 2.0 ** 40, 0, True, True, "p")), b
        one = rg.gQ.NewPoly()
        rg.enc.Encode(z[b], one, Scale=2.0 ** 40, LogSlots=ls, IsNTT=True, IsMontgomery=True)
        assert eq(one.get(), gq[b]), b  # batch 3 equals three single calls
    # without a P side
    rg.enc.EncodeQP(z, pq, None, Scale=2.0 ** 40, LogSlots=ls, IsMontgomery=False)
    assert eq(pq.download()[2], rg.want_words(z[2], ls, 2.0 ** 40, 1, True, False, "q"))


def test_encode_above_the_one_workgroup_threshold(ctx):
    """the separate quantiser after the multi-pass transform, one limb"""
    th = Rig(ctx, 6, 1).enc.FFTOneWorkgroupMaxLogN
    rg = Rig(ctx, th + 2, 1)
    rng = rng_for(5700)
    n = 1 << (th + 1)
    z = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
    pt = rg.gQ.NewPoly()
    rg.enc.Encode(z, pt, Scale=2.0 ** 40, IsNTT=False)
    assert eq(pt.get(), rg.want_words(z, th + 1, 2.0 ** 40, 0, False, False))


# ---- Decode ----------------------------------------------------------------------------------------------------------------------
def residues(xs, mods, N):
    w = np.zeros((len(mods), N), dtype=np.uint64)
    for i, x in enumerate(xs):
        for l, q in enumerate(mods):
            w[l, i] = x % q
    return w


@pytest.mark.parametrize("nlimbs", [2, 32])
def test_reconstruction_edge_list(ctx, nlimbs):
    """is_ntt = 0, not batched: every coefficient; 2 limbs of 55 bits and the cap"""
    rg = Rig(ctx, 6, nlimbs)
    assert rg.enc.DecodeMaxLimbs == 32
    Q = math.prod(rg.q)
    xs = R.reconstruction_cases(Q)
    pt = rg.gQ.NewPoly().upload(residues(xs, rg.q, rg.N))
    for scale in (1.0, 2.0 ** 20, 3.0):
        got = rg.enc.Decode(pt, Scale=scale, IsBatched=False, IsNTT=False, complex_out=False)[0]
        want = np.array([R.coeff_to_float([x % q for q in rg.q], rg.q, scale) for x in xs])
        assert eq(got[: len(xs)], want), scale
        assert not got[len(xs):].any()
    gc = rg.enc.Decode(pt, Scale=1.0, IsBatched=False, IsNTT=False, complex_out=True)[0]
    assert eq(gc.real, rg.enc.Decode(pt, Scale=1.0, IsBatched=False, IsNTT=False, complex_out=False)[0]) and not gc.imag.any()
    # every instantiation of the kernel below the cap, on the levels of the same ring
    for level in sorted({0, 1, 2, 3, 4, 7, 8, 15, 16, nlimbs - 1} & set(range(nlimbs))):
        mods = rg.q[: level + 1]
        Ql = math.prod(mods)
        xl = R.reconstruction_cases(Ql) if Ql > 2 ** 103 else [0, 1, -1, (Ql >> 1) - 1, Ql >> 1, Ql - 1, 2 ** 53 + 1, -(2 ** 53 + 1)]
        pl = la.Poly(rg.gQ, level + 1, 1).upload(residues(xl, mods, rg.N))
        got = rg.enc.Decode(pl, Scale=2.0, IsBatched=False, IsNTT=False, complex_out=False, level=level)[0]
        assert eq(got[: len(xl)], np.array([R.coeff_to_float([x % q for q in mods], mods, 2.0) for x in xl])), level


def test_decode_rejects_more_limbs_than_the_cap(ctx):
    rg = Rig(ctx, 6, 33)
    pt = rg.gQ.NewPoly()
    assert rg.enc.Decode(pt, Scale=1.0, IsBatched=False, IsNTT=False, level=31).shape == (1, 64)
    with pytest.raises(la.HeringError) as e:
        rg.enc.Decode(pt, Scale=1.0, IsBatched=False, IsNTT=False, level=32)
    assert e.value.code == -1 and "32" in str(e.value)


@pytest.mark.parametrize("ci", [False, True])
def test_decode_random_plaintexts(ctx, ci):
    """levels 0, 1 and top; NTT and coefficient domain; batched (full and sparse, the conjugate-invariant fold) and coefficient
    encodings; logprec = 20; batch 2"""
    rg = Rig(ctx, 7, 3, ci=ci)
    rng = rng_for(5800 + ci)
    scale = 2.0 ** 30
    for level in (0, 1, 2):
        mods = rg.q[: level + 1]
        Q = math.prod(mods)
        # coefficients of about 50 bits around 0 mod Q, so that the slot values are of order 2^20 / scale
        small = rng.integers(-(1 << 50), 1 << 50, (2, rg.N))
        coef = np.stack([residues([int(x) for x in small[b]], mods, rg.N) for b in range(2)])
        for ntt in (False, True):
            up = np.stack([rg.oQ.NTT(coef[b], level=level) for b in range(2)]) if ntt else coef
            pt = la.Poly(rg.gQ, level + 1, 2).upload(up)
            for log_slots in (rg.max_log_slots, 2, 0):
                for logprec in (0.0, 20.0):
                    got = rg.enc.DecodePublic(pt, Scale=scale, logprec=logprec, LogSlots=log_slots, IsNTT=ntt, level=level)
                    gr = rg.enc.DecodePublic(pt, Scale=scale, logprec=logprec, LogSlots=log_slots, IsNTT=ntt, level=level, complex_out=False)
                    for b in range(2):
                        wr, wi = R.decode_slots(coef[b], mods, scale, log_slots, rg.N, ci, rg.M, rg.rre, rg.rim, logprec)
                        assert eq(got[b].real, wr) and eq(got[b].imag, wi), (level, ntt, log_slots, logprec, b)
                        assert eq(gr[b], wr)
            got = rg.enc.Decode(pt, Scale=scale, IsBatched=False, IsNTT=ntt, level=level, complex_out=False)
            for b in range(2):
                want = np.array([R.coeff_to_float(coef[b][:, i], mods, scale) for i in range(rg.N)])
                assert eq(got[b], want), (level, ntt, b)
            assert eq(pt.download(), up)  # the plaintext is not changed
    if ci:  # the fold on its own: before the transform the imaginary part of slot i is minus the real part of slot slots - i
        wr, wi = R.decode_slots(coef[0], mods, scale, 3, rg.N, True, rg.M, rg.rre, rg.rim, fft=False)
        assert wi[0] == 0 and eq(wi[1:], -wr[1:][::-1])


@pytest.mark.parametrize("ci", [False, True])
def test_round_trip_on_the_device(ctx, ci):
    """schemes/ckks/ckks_test.go:278-283: log2(1 / err) >= log2(scale) - (logN + 2)"""
    rg = Rig(ctx, 10, 2, ci=ci)
    rng = rng_for(5900 + ci)
    for log_slots, log_scale in ((rg.max_log_slots, 45), (4, 30)):
        n = 1 << log_slots
        z = rng.uniform(-1, 1, (2, n)) + (0 if ci else 1j * rng.uniform(-1, 1, (2, n)))
        pt = la.Poly(rg.gQ, 2, 2)
        rg.enc.Encode(z, pt, Scale=2.0 ** log_scale, LogSlots=log_slots)
        back = rg.enc.Decode(pt, Scale=2.0 ** log_scale, LogSlots=log_slots)
        err = max(np.max(np.abs(back.real - z.real)), np.max(np.abs(back.imag - np.imag(z))))
        assert math.log2(1 / err) >= log_scale - (rg.logN + 2), (log_slots, err)


# ---- rejections, launches, scheduling ------------------------------------------------------------------------------------------
def test_rejections_leave_every_operand_unchanged(ctx):
    rg = Rig(ctx, 6, 2, npp=1)
    other = Rig(ctx, 7, 2)
    rng = rng_for(6000)
    pt = rg.gQ.NewPoly().upload(rng.integers(0, 1 << 50, (2, 64), dtype=np.uint64))
    pp = rg.gP.NewPoly().upload(rng.integers(0, 1 << 50, (1, 64), dtype=np.uint64))
    before, before_p = pt.download(), pp.download()
    z = rng.uniform(-1, 1, 32) + 1j * rng.uniform(-1, 1, 32)
    e = rg.enc
    bad = z.copy()
    bad[5] = complex(0, math.inf)
    nan = z.copy()
    nan[0] = math.nan
    no_p = ckks.Encoder(rg.gQ)
    L, f64p = _lib.load(), ctypes.POINTER(ctypes.c_double)
    raw = lambda fn, *a: _lib.check(fn(*a))
    zp = np.ascontiguousarray(z).view(np.float64).ctypes.data_as(f64p)
    wide = np.zeros(2 * 65536).ctypes.data_as(f64p)
    ctx2 = la.Context(0)
    ring2, ring2p = la.Ring(ctx2, rg.N, rg.q), la.Ring(ctx2, rg.N, rg.p)
    foreign, foreign_p = ring2.NewPoly(), ring2p.NewPoly()
    many = la.Poly(rg.gQ, 1, 65536)
    calls = [
        lambda: e.Encode(z, pt, Scale=2.0 ** 30, level=2),                       # a level the ring lacks
        lambda: e.Encode(z, pt, Scale=2.0 ** 30, level=-1),
        lambda: e.Encode(z, pt, Scale=2.0 ** 30, LogSlots=6),                    # logSlots out of [0, LogMaxDimensions]
        lambda: e.Encode(z, pt, Scale=2.0 ** 30, LogSlots=-1),
        lambda: e.Encode(z, pt, Scale=2.0 ** 30, LogSlots=4),                    # too many values
        lambda: e.Encode(np.ones(65), pt, Scale=2.0 ** 30, IsBatched=False),
        lambda: e.Encode(z, pt, Scale=2.0 ** 30, IsBatched=False),               # complex values of a coefficient encode
        lambda: e.Encode(bad, pt, Scale=2.0 ** 30),                              # non-finite inputs
        lambda: e.Encode(nan, pt, Scale=2.0 ** 30),
        lambda: e.Encode(z, pt, Scale=math.inf),
        lambda: e.Encode(z, other.gQ.NewPoly(), Scale=2.0 ** 30),                # a polynomial of another degree
        lambda: e.Encode(z, la.Poly(rg.gQ, 1, 1), Scale=2.0 ** 30, level=1),     # too few limbs
        lambda: e.Encode(np.stack([z, z]), pt, Scale=2.0 ** 30),                 # batch mismatch
        lambda: no_p.EncodeQP(z, pt, pp, Scale=2.0 ** 30),                       # no ringP
        lambda: e.EncodeQP(z, pt, pp, Scale=2.0 ** 30, levelP=1),
        lambda: e.Decode(pt, Scale=2.0 ** 30, level=2),
        lambda: e.Decode(pt, Scale=2.0 ** 30, LogSlots=6),
        lambda: e.Decode(pt, Scale=0.0),
        lambda: e.Decode(other.gQ.NewPoly(), Scale=2.0 ** 30),
        lambda: e._fft(np.zeros(64, dtype=complex), 6, False),                 # logn above LogMaxDimensions
        lambda: e.IFFT(bad, 5),
        lambda: e.EncodeQP(z, pt, pt, Scale=2.0 ** 30, levelP=0),                # outP is outQ
        lambda: e.Encode(np.zeros(0), pt, Scale=2.0 ** 30),                      # n_values = 0
        lambda: raw(L.he_ckks_encode, e.h, 1, 5, 2.0 ** 30, 1, 1, 0, None, 32, 1, 1, pt.h),   # values NULL
        lambda: raw(L.he_ckks_encode_qp, e.h, 1, 0, 5, 2.0 ** 30, 1, 1, None, 32, 1, 1, pt.h, pp.h),
        lambda: e.Encode(z, foreign, Scale=2.0 ** 30),                           # a polynomial of another context
        lambda: e.EncodeQP(z, pt, foreign_p, Scale=2.0 ** 30),
        lambda: e.Decode(foreign, Scale=2.0 ** 30),
        lambda: e.Encode(np.ones((65536, 1)), pt, Scale=2.0 ** 30, LogSlots=0),  # batch above 65535
        lambda: raw(L.he_ckks_encode, e.h, 1, 5, 2.0 ** 30, 1, 1, 0, zp, 32, 1, 0, pt.h),     # batch 0
        lambda: e.Decode(many, Scale=2.0 ** 30, level=0),                        # more than 65535 entries
        lambda: e.Decode(pt, Scale=math.inf),                                    # a non-finite decode scale or logprec
        lambda: e.Decode(pt, Scale=math.nan),
        lambda: e.DecodePublic(pt, Scale=2.0 ** 30, logprec=math.nan),
        lambda: e.DecodePublic(pt, Scale=2.0 ** 30, logprec=math.inf),
        lambda: raw(L.he_ckks_decode, e.h, 1, 5, 2.0 ** 30, 1, 1, 0.0, pt.h, 1, None),        # values NULL
        lambda: raw(L.he_ckks_fft, e.h, 0, 0, wide),                             # a bad batch of the transforms
        lambda: raw(L.he_ckks_ifft, e.h, 0, 65536, wide),
        lambda: raw(L.he_ckks_fft, e.h, 0, -1, wide),
        lambda: raw(L.he_ckks_ifft, e.h, 5, 1, None),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(la.HeringError) as err:
            call()
        assert err.value.code == -1, (i, str(err.value))
        assert eq(pt.download(), before) and eq(pp.download(), before_p), i
    with pytest.raises(la.HeringError):
        ckks.Encoder(rg.gQ, other.gQ)  # ringP of another degree
    with pytest.raises(la.HeringError):
        ckks.Encoder(rg.gQ, ring2p)    # ... of another context
    assert "logSlots" in str(pytest.raises(la.HeringError, lambda: e.Encode(z, pt, Scale=1.0, LogSlots=9)).value)
    x, y = rg.gQ.NewPoly(), rg.gQ.NewPoly()
    rg.gQ.NTT(x, y)
    ctx.sync()
    with ctx.capture():
        rg.gQ.NTT(x, y)
        with pytest.raises(la.HeringError):
            e.Encode(z, pt, Scale=2.0 ** 30)  # host transfers cannot be captured
    assert eq(pt.download(), before)
    e.Encode(z, pt, Scale=2.0 ** 30)
    assert eq(pt.get(), rg.want_words(z, 5, 2.0 ** 30, 1, True, False))


def census(ctx, call):
    ctx.sync()
    ctx.prof_begin()
    call()
    ctx.sync()
    return {k: v[0] for k, v in ctx.prof_end().items()}


def test_launch_census(ctx):
    """one fused launch for iFFT + quantise at one-workgroup sizes, whatever the batch and the number of limbs; then the existing
    NTT and MForm launches"""
    rg = Rig(ctx, 10, 3, npp=1)
    rng = rng_for(6100)
    z = rng.uniform(-1, 1, (3, 512)) + 1j * rng.uniform(-1, 1, (3, 512))
    pq, pp = la.Poly(rg.gQ, 3, 3), la.Poly(rg.gP, 1, 3)
    ntt_q = census(ctx, lambda: rg.gQ.NTT(pq, pq))
    ntt_p = census(ctx, lambda: rg.gP.NTT(pp, pp))
    c = census(ctx, lambda: rg.enc.Encode(z, pq, Scale=2.0 ** 40, IsNTT=False))
    assert c == {"special_ifft_quantize": 1}, c
    c = census(ctx, lambda: rg.enc.EncodeQP(z, pq, pp, Scale=2.0 ** 40, IsNTT=True, IsMontgomery=True))
    assert c.pop("special_ifft_quantize") == 1 and c.pop("ew") == 2, c
    assert sum(c.values()) == sum(ntt_q.values()) + sum(ntt_p.values()) and set(c) == set(ntt_q) | set(ntt_p), (c, ntt_q, ntt_p)
    c = census(ctx, lambda: rg.enc.Decode(pq, Scale=2.0 ** 40, IsNTT=False))
    assert c == {"rns_to_f64": 1, "special_fft": 1}, c
    c = census(ctx, lambda: rg.enc.Encode(z.real, pq, Scale=2.0 ** 40, IsBatched=False, IsNTT=False))
    assert c == {"f64_to_rns": 1}, c


@pytest.mark.parametrize("deferred", [0, 4])
def test_order_with_the_submission_queue(ctx, deferred):
    """an encode runs after the queued writers of its output, a decode after those of its input (he_poly_upload's rule)"""
    rg = Rig(ctx, 10, 2)
    rng = rng_for(6200 + deferred)
    z = rng.uniform(-1, 1, 256) + 1j * rng.uniform(-1, 1, 256)
    x = rg.gQ.NewPoly().upload(rng.integers(0, 1 << 50, (2, 1024), dtype=np.uint64))
    pt, tmp = rg.gQ.NewPoly(), rg.gQ.NewPoly()
    want = rg.want_words(z, 8, 2.0 ** 40, 1, True, False)
    ctx.SetCoalescing(64, 500)
    if deferred:
        ctx.SetDeferred(deferred)
    try:
        for _ in range(3):
            rg.gQ.NTT(x, pt)                                  # a queued writer of the encode's output
            rg.enc.Encode(z, pt, Scale=2.0 ** 40, LogSlots=8)
            assert eq(pt.get(), want)
            rg.gQ.NTT(x, tmp)
            rg.gQ.INTT(pt, tmp)                               # a queued writer of the decode's input
            got = rg.enc.Decode(tmp, Scale=2.0 ** 40, LogSlots=8, IsNTT=False)[0]
            wr, wi = R.decode_slots(rg.oQ.INTT(want), rg.q, 2.0 ** 40, 8, rg.N, False, rg.M, rg.rre, rg.rim)
            assert eq(got.real, wr) and eq(got.imag, wi)
    finally:
        if deferred:
            ctx.SetDeferred(0)
        ctx.SetCoalescing(0, 0)


def test_encode_inside_a_recorded_window_fails_trace_end(ctx):
    rg = Rig(ctx, 6, 1)
    pt = rg.gQ.NewPoly()
    z = np.ones(32, dtype=complex)
    _lib.trace_begin()
    try:
        rg.enc.Decode(pt, Scale=1.0)
        rg.enc.FFT(z, 5)
        rg.enc.Roots()
        prog = _lib.trace_end()
        assert prog.size == 0
        _lib.trace_begin()
        rg.enc.Encode(z, pt, Scale=2.0 ** 20)
        with pytest.raises(RuntimeError, match="he_ckks_encode"):
            _lib.trace_end()
    finally:
        if _lib._trace is not None:
            try:
                _lib.trace_end()
            except RuntimeError:
                pass


def poison_case():
    """run by test_encode_writes_every_output_word in a process of its own with HERING_POISON=1: the outputs are scratch polynomials"""
    c = la.Context(0)
    rng = rng_for(6300)
    for ci in (False, True):
        rg = Rig(c, 8, 2, ci=ci, npp=1)
        for ls in (rg.max_log_slots, 2):
            z = rng.uniform(-1, 1, 1 << ls) + 1j * rng.uniform(-1, 1, 1 << ls)
            pq, pp = la.Poly(rg.gQ, 2, 1, zero=False), la.Poly(rg.gP, 1, 1, zero=False)
            for ntt in (False, True):
                rg.enc.EncodeQP(z, pq, pp, Scale=2.0 ** 40, LogSlots=ls, IsNTT=ntt, IsMontgomery=False)
                assert eq(pq.get(), rg.want_words(z, ls, 2.0 ** 40, 1, ntt, False, "q")), (ci, ls, ntt)
                assert eq(pp.get(), rg.want_words(z, ls, 2.0 ** 40, 0, ntt, False, "p")), (ci, ls, ntt)
            got = rg.enc.Decode(pq, Scale=2.0 ** 40, LogSlots=ls)[0]
            wr, wi = R.decode_slots(rg.oQ.INTT(pq.get()), rg.q, 2.0 ** 40, ls, rg.N, ci, rg.M, rg.rre, rg.rim)
            assert eq(got.real, wr) and eq(got.imag, wi), (ci, ls)
        pt = la.Poly(rg.gQ, 2, 1, zero=False)
        rg.enc.Encode(z.real[:3], pt, Scale=2.0 ** 40, IsBatched=False, IsNTT=False)
        assert eq(pt.get(), R.quantise_poly(z.real[:3], 2.0 ** 40, rg.q, rg.N))
    print("poison OK")


def test_encode_writes_every_output_word(ctx):
    env = dict(os.environ, HERING_POISON="1")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c",
                        "import tests.conftest; from tests.test_gpu_ckks_encoder import poison_case; poison_case()"],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "poison OK" in r.stdout
