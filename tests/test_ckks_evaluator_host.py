"""include/hering_ckks_evaluator.h and lattigo_amd's rlwe.Scale without a device: the header's symbols, the replay numbers and the
profiler names; rlwe.Scale against exact rational arithmetic rounded to 128 bits (random operands and constructed ties) and
against the integer-only restatement of tests/ckks_evaluator_ref.py; the mirror's scalar words against the oracle evaluator's;
the restatement of the four entries over the oracle's ring primitives against plain modular arithmetic."""
import random
from fractions import Fraction

import numpy as np
import pytest

import __graft_entry__ as graft
from lattigo_amd import _lib
from lattigo_amd import polyeval as NP
from lattigo_amd.rlwe import MetaData, NewScale, Scale
from oracle import circuits as OC
from oracle import oracle as O
from tests import boundary as Bd
from tests import ckks_evaluator_ref as REF
from tests.conftest import Pi60, Qi60
from tests.helpers import rng_for

NEW = ["he_ckks_add", "he_ckks_scalar", "he_ckks_mul_pt", "he_ckks_mul_relin_then_add"]


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


def test_header_symbols_replay_numbers_and_kernel_names(lib):
    syms = _lib.declared_symbols()
    assert all(s in syms and hasattr(lib, s) for s in NEW)
    last = max(v[0] for v in _lib._TRACE_FNS_LINTRANS.values())
    assert sorted(_lib._TRACE_FNS_CKKS_EVALUATOR[s][0] for s in NEW) == list(range(last + 1, last + 5))
    assert set(_lib._TRACE_FNS_CKKS_EVALUATOR) == set(NEW) and not any(s in _lib._TRACE_IGNORE for s in NEW)
    for s in NEW:  # every array argument of a recorded call has its length
        kinds = _lib._TRACE_FNS_CKKS_EVALUATOR[s][1]
        assert len(kinds) == len(getattr(lib, s).argtypes)
        assert all((s, k) in _lib._TRACE_LEN for k, c in enumerate(kinds) if c in "AH")
    names = [lib.he_prof_kernel_name(i).decode() for i in range(64)]
    assert names[names.index("poly_leaf_group") + 1: names.index("poly_leaf_group") + 3] == ["ct_lin", "tensor_add"]  # appended


def test_entries_fail_loudly_without_a_device(lib):
    """no device, no fallback: a bad ring handle is HE_EHANDLE before anything else is looked at"""
    h = (_lib.H * 1)(0)
    assert lib.he_ckks_add(0, 0, 0, 1, h, 1, h, 0, None, 1, h) == -2
    assert lib.he_ckks_mul_relin_then_add(0, 0, 0, 0, 0, 0, 0, None, 0, 0, 0) == -2


# ---- rlwe.Scale ----------------------------------------------------------------------------------------------------------------------------
def _round128(x: Fraction) -> Fraction:
    """x > 0 rounded to 128 significant bits, ties to even, by integer arithmetic"""
    e = x.numerator.bit_length() - x.denominator.bit_length() - 128
    for e in (e - 1, e, e + 1):
        m, r = divmod(x.numerator * (1 << max(-e, 0)), x.denominator * (1 << max(e, 0)))
        if m.bit_length() == 128:
            break
    den = x.denominator * (1 << max(e, 0))
    if 2 * r > den or (2 * r == den and m & 1):
        m += 1
    return Fraction(m) * Fraction(2) ** e


def test_scale_mul_div_round_to_128_bits_nearest_even():
    rnd = random.Random(0x5CA1E)
    for _ in range(1500):
        a = rnd.getrandbits(rnd.randint(1, 190)) + 1
        b = rnd.getrandbits(rnd.randint(1, 190)) + 1
        x, y, rx, ry = Scale(a), Scale(b), REF.Scale(a), REF.Scale(b)
        assert x.Value == _round128(Fraction(a)) == rx.fraction()
        for op, exact in (("Mul", x.Value * y.Value), ("Div", x.Value / y.Value)):
            got, ref = getattr(x, op)(y), getattr(rx, op)(ry)
            assert got.Value == _round128(exact) == ref.fraction(), (op, a, b)
            assert got.Int() == ref.Int() == _round128(exact).numerator // _round128(exact).denominator
            assert got.Float64() == ref.Float64()
        assert x.Cmp(y) == rx.Cmp(ry) == (x.Value > y.Value) - (x.Value < y.Value)
        assert x.Max(y).Value == max(x.Value, y.Value) and x.Min(y).Value == min(x.Value, y.Value)
    assert Scale(0.1).Value == Fraction(0.1) and NewScale(Scale(3)).Value == 3 and Scale(2.5).Int() == 2 and Scale(1 << 70).Uint64() == (1 << 64) - 1


def test_scale_ties_go_to_even():
    """products exactly half-way between two 128-bit floats: (2^127 + k) * 2 with an odd last bit added below the mantissa"""
    for k in (0, 1, 2, 3, 0x1234567):
        m = (1 << 127) + k
        tie = Fraction(2 * m + 1)  # 129 bits, the lowest one set: half-way between m and m + 1 (times 2)
        want = Fraction(2 * (m if m % 2 == 0 else m + 1))
        assert _round128(tie) == want
        # as a product: (2 m + 1) = a * b exactly, both factors below 2^128
        a, b = Fraction(2 * m + 1, 3), Fraction(3)
        if a.denominator == 1:
            assert Scale(a).Mul(b).Value == want == REF.Scale(a).Mul(b).fraction()
        # as a quotient: (2 m + 1) 2^64 / 2^64
        assert Scale((2 * m + 1) << 3).Value == want * 8  # the constructor rounds the same way
    x = Scale(Fraction((1 << 128) + 1, 1 << 64))  # 129 significant bits: rounds to 2^64 (even)
    assert x.Value == Fraction(1 << 64) and REF.Scale(Fraction((1 << 128) + 1, 1 << 64)).fraction() == x.Value
    y = Scale(Fraction((1 << 128) + 3, 1 << 64))  # half-way above an odd mantissa: up
    assert y.Value == Fraction((1 << 128) + 4, 1 << 64)


def test_metadata_copy_is_independent():
    m = MetaData(1 << 40, LogDimensions=(0, 9))
    c = m.copy()
    c.Scale = c.Scale.Mul(3)
    assert m.Scale.Value == 1 << 40 and c.Scale.Value == 3 << 40 and c.LogDimensions == (0, 9) and c.IsNTT and c.IsBatched


# ---- scalar words ------------------------------------------------------------------------------------------------------------------------
def test_scalar_words_of_the_mirror_equal_the_oracle_evaluators():
    N, q = 1 << 10, Qi60[:3]
    oQ = O.Ring(N, q)
    oe = OC.CKKSCtEvaluator(O.Evaluator(oQ, O.Ring(N, Pi60[:2])), None, float(1 << 45))
    sch = NP.CKKSScheme(q, [int(oQ.roots_forward(i)[1]) * pow(1 << 64, -1, m) % m for i, m in enumerate(q)], float(1 << 45))
    for c in (0.5, 3, -2.25 + 1.5j, Fraction(1, 3), 7, Fraction(3 << 45), -1, 1e-9, 12345.678 - 0.001j):
        for scale in (1, q[2], Fraction(1 << 45), Fraction(3), Scale(q[2]).Mul(q[1]).Value):
            a, b = oe._rns(2, scale, c), sch._rns(2, Fraction(scale), c)
            assert [int(x) for x in a[0]] == b[0] and [int(x) for x in a[1]] == b[1], (c, scale)
        assert oe._is_int(c) == sch._is_int(c)


# ---- the restatement of the entries against plain arithmetic ---------------------------------------------------------------------------------
@pytest.mark.parametrize("logN", [4, 9])
def test_restatement_of_the_entries_equals_modular_arithmetic(logN):
    N = 1 << logN
    q = [Bd.class_chain(logN, "h")[0], Bd.primes_below(36, logN + 1, 1)[0], Bd.class_chain(logN, "I")[0]]
    o, rng = O.Ring(N, q), rng_for(13300 + logN)
    kinds = ("uniform", "max", "zero")

    def ct(n):
        out = []
        for _ in range(n):
            kind = kinds[int(rng.integers(0, 3))]
            out.append(np.zeros((3, N), dtype=np.uint64) if kind == "zero" else np.stack([Bd.word_row(kind, rng, m, N) for m in q]))
        return out

    eq = lambda x, y: len(x) == len(y) and all(np.array_equal(u, v) for u, v in zip(x, y))
    for level in (2, 1, 0):
        for words in ([m - 1 for m in q], [0, 0, 0], [1, 1, 1], [int(rng.integers(0, m)) for m in q]):
            w = np.array(words, dtype=np.uint64)
            s1 = np.array([int(rng.integers(0, m)) for m in q], dtype=np.uint64)
            for sub in (False, True):
                for n0 in (1, 2, 3):
                    for n1 in (1, 2, 3):
                        for sc in (0, 1, 2):
                            a, b = ct(n0), ct(n1)
                            assert eq(REF.ckks_add(o, level, sub, a, b, sc, w), REF.exact_add(o, level, sub, a, b, sc, w)), (level, sub, n0, n1, sc)
            for op in range(4):
                for pre in ((None, w) if op == 3 else (None,)):
                    a, out = ct(3), ct(3)
                    assert eq(REF.ckks_scalar(o, level, op, a, w, s1, out, pre), REF.exact_scalar(o, level, op, a, w, s1, out, pre)), (level, op)
            a, out, pt = ct(3), ct(3), ct(1)[0]
            for oo, pre in ((None, None), (out, None), (out, w)):
                assert eq(REF.ckks_mul_pt(o, level, a, pt, oo, pre), REF.exact_mul_pt(o, level, a, pt, oo, pre))
            a, b, out = ct(2), ct(2), ct(3)
            for pre in (None, w):
                assert eq(REF.ckks_mul_relin_then_add(o, level, a, b, out, pre), REF.exact_mul_then_add(o, level, a, b, out, pre))


# ---- the restatement decrypts correctly: real keys on the oracle, every method and operand kind ---------------------------------------------
class _Noise:
    """The bound, derived from the parameters.  A tracked value is (message bound M, variance V of a slot's error, in message
    units).  Coefficient noise of variance v at scale s is slot noise of variance N v / s^2 (a slot is a sum of the N coefficients
    times numbers of modulus 1).  Fresh under sk: v = sigma^2 + 1/12 (the Gaussian error, sigma = 3.2, and the rounding of the
    encoding).  Rounding by a rescale, and the rounding at the end of a key switch (whose own term, beta N sigma^2 D^2 / (12 P^2)
    with digits D < 2^100 and P > 2^109, is below 1): v = (1 + 2 N / 3) / 12 + 1, a uniform rounding on c0 and one on c1 times the
    ternary secret of variance 2 / 3.  Amplification: a sum adds variances; a product with a message bounded by M multiplies a
    variance by M^2 (both cross terms are counted); a constant encoded at scale s is off by at most 1/2 in each part, (1 / 2) / s^2
    per product.  The check is six standard deviations."""
    SIGMA2 = 3.2 ** 2

    def __init__(self, N):
        self.N = N
        self.round = (1 + 2 * N / 3) / 12 + 1

    def fresh(self, scale, M=2 ** 0.5):
        return (M, self.N * (self.SIGMA2 + 1 / 12) / scale ** 2)

    def plain(self, scale, M=2 ** 0.5):
        return (M, self.N / 12 / scale ** 2)

    def add(self, a, b):
        return (a[0] + b[0], a[1] + b[1])

    def const(self, a, c, scale):
        return (a[0] + abs(c), a[1] + 0.5 / scale ** 2)

    def mul(self, a, b):
        return (a[0] * b[0], a[1] * b[0] ** 2 + b[1] * a[0] ** 2 + a[1] * b[1])

    def mulc(self, a, c, scale):
        return (a[0] * abs(c), a[1] * abs(c) ** 2 + a[0] ** 2 * 0.5 / scale ** 2)

    def rounded(self, a, scale):  # a rescale to `scale`, or a key switch at `scale`
        return (a[0], a[1] + self.N * self.round / scale ** 2)


@pytest.fixture(scope="module")
def hostrig():
    from tests import rlwe_fixtures as F
    logN = 9
    N = 1 << logN
    q, p = O.GenModuli(logN + 1, [55, 45, 45, 45], [55, 55])
    oQ, oP = O.Ring(N, q), O.Ring(N, p)
    rng = rng_for(13800)
    sk = F.SecretKey(rng, oQ, oP)
    rlk = F.gen_evaluation_key(rng, oQ, oP, oQ.binop("MulCoeffsMontgomery", sk.Q, sk.Q), sk)
    from lattigo_amd.rlwe import GaloisElementsForInnerSum
    g1 = pow(5, 1, 2 * N)
    galels = sorted({g1, pow(5, 3, 2 * N), 2 * N - 1} | set(GaloisElementsForInnerSum(2 * N, 1, 4)) | set(GaloisElementsForInnerSum(2 * N, 2, 3)))
    gks = F.gen_galois_keys(rng, oQ, oP, sk, galels)
    swk = F.gen_evaluation_key(rng, oQ, oP, sk.Q, sk)
    S = float(1 << 45)
    enc = lambda values, level, scale: F.ckks_encode(values, N, scale, q[: level + 1])
    ev = REF.RefEvaluator(O.Evaluator(oQ, oP), S, rlk, gks, enc)
    return dict(N=N, q=q, oQ=oQ, sk=sk, rng=rng, ev=ev, S=1 << 45, F=F, noise=_Noise(N), swk=swk)


def _decrypt(rg, ct):
    """the phase c0 + c1 s (+ c2 s^2), centred and divided by the scale, in the slots"""
    F, level = rg["F"], ct.Level()
    r = O.Ring(rg["N"], rg["q"][: level + 1])
    s = rg["sk"].Q[: level + 1]
    acc, sp = ct.Value[0][: level + 1], s
    for c in ct.Value[1:]:
        acc = r.binop("Add", acc, r.binop("MulCoeffsMontgomery", c[: level + 1], sp))
        sp = r.binop("MulCoeffsMontgomery", sp, s)  # the next power of s: the product of two Montgomery forms is one
    zero = np.zeros_like(acc)
    return F.ckks_decrypt(r, np.stack([acc, zero]), rg["sk"], ct.Scale.fraction())


def _fresh(rg, z, scale, level=None):
    level = len(rg["q"]) - 1 if level is None else level
    r = O.Ring(rg["N"], rg["q"][: level + 1])
    ct = rg["F"].ckks_encrypt(rg["rng"], r, rg["sk"], z, float(scale))
    return REF.RefCt(list(ct), scale, 8)


def _check(rg, ct, want, track, tag):
    got = _decrypt(rg, ct)
    err, bound = float(np.max(np.abs(got - want))), 6 * track[1] ** 0.5
    print(tag, "level", ct.Level(), "error", err, "bound", bound)
    assert err <= bound, (tag, err, bound)
    assert float(np.max(np.abs(want))) <= track[0] + 1e-9, tag


def test_restatement_decrypts_every_method_and_operand_kind(hostrig):
    rg = hostrig
    ev, S, nz, rng, N, q = rg["ev"], rg["S"], rg["noise"], rg["rng"], rg["N"], rg["q"]
    top = len(q) - 1
    vec = lambda: rng.uniform(-1, 1, N // 2) + 1j * rng.uniform(-1, 1, N // 2)
    x, y, z, w, v = vec(), vec(), vec(), vec(), vec()
    a, b, a2 = _fresh(rg, x, S), _fresh(rg, y, 3 * S), _fresh(rg, z, S)
    ptw = REF.RefCt([rg["F"].ckks_encode(w, N, float(S), q)], S, 8)
    na, nb, na2, nw = nz.fresh(S), nz.fresh(3 * S), nz.fresh(S), nz.plain(S)
    new = lambda d=1, lvl=top: ev.NewCiphertext(d, lvl)
    _check(rg, a, x, na, "fresh")
    # Add / Sub: ciphertext (both directions of the scale matching), plaintext, scalar, vector
    for name, f in (("Add", lambda p, r_: p + r_), ("Sub", lambda p, r_: p - r_)):
        o = new()
        getattr(ev, name)(a, b, o)
        _check(rg, o, f(x, y), nz.add(na, nb), name + " ct")
        assert o.Scale.fraction() == 3 * S
        o = new()
        getattr(ev, name)(b, a, o)
        _check(rg, o, f(y, x), nz.add(na, nb), name + " ct, op0 larger")
        o = new()
        getattr(ev, name)(a, ptw, o)
        _check(rg, o, f(x, w), nz.add(na, nw), name + " pt")
        o = new()
        getattr(ev, name)(a, 0.5 - 2j, o)
        _check(rg, o, f(x, 0.5 - 2j), nz.const(na, 0.5 - 2j, S), name + " scalar")
        o = new()
        getattr(ev, name)(a, v, o)
        _check(rg, o, f(x, v), nz.add(na, nz.plain(S)), name + " vector")
    # Mul: scalar (a non-integer is encoded at q_level; an integer multiplies as it is), vector, plaintext, ciphertext
    qt = float(q[top])
    o = new()
    ev.Mul(a, 0.37 + 0.1j, o)
    assert o.Scale.fraction() == REF.Scale(S).Mul(q[top]).fraction()
    t = nz.mulc(na, 0.37 + 0.1j, qt)
    _check(rg, o, x * (0.37 + 0.1j), t, "Mul scalar")
    r1 = new(1, top)
    ev.Rescale(o, r1)
    assert r1.Level() == top - 1
    _check(rg, r1, x * (0.37 + 0.1j), nz.rounded(t, r1.Scale.Float64()), "Rescale")
    o = new()
    ev.Mul(a, 3, o)
    assert o.Scale.fraction() == S
    _check(rg, o, 3 * x, nz.mulc(na, 3, float("inf")), "Mul integer")
    o = new()
    ev.Mul(a, v, o)
    _check(rg, o, x * v, nz.mul(na, nz.plain(qt)), "Mul vector")
    o = new()
    ev.Mul(a, ptw, o)
    _check(rg, o, x * w, nz.mul(na, nw), "Mul pt")
    o2 = new(2)
    ev.Mul(a, a2, o2)
    tm = nz.mul(na, na2)
    _check(rg, o2, x * z, tm, "Mul ct (degree 2)")
    o = new()
    ev.Relinearize(o2, o)
    _check(rg, o, x * z, nz.rounded(tm, S * S), "Relinearize")
    o = new()
    ev.MulRelin(a, a2, o)
    _check(rg, o, x * z, nz.rounded(tm, S * S), "MulRelin")
    # MulThenAdd: scalar with equal scales (the accumulator is multiplied by q_level), with a larger accumulator scale, an integer;
    # vector; plaintext; ciphertext with and without relinearization and with the scale-up of the accumulator
    acc = a.CopyNew()
    ev.MulThenAdd(a2, 0.25, acc)
    assert acc.Scale.fraction() == REF.Scale(S).Mul(q[top]).fraction()
    _check(rg, acc, x + 0.25 * z, nz.add(na, nz.mulc(na2, 0.25, qt)), "MulThenAdd scalar, equal scales")
    acc = b.CopyNew()
    ev.MulThenAdd(a2, 0.25, acc)
    assert acc.Scale.fraction() == 3 * S
    _check(rg, acc, y + 0.25 * z, nz.add(nb, nz.mulc(na2, 0.25, 3.0)), "MulThenAdd scalar, larger accumulator")
    acc = a.CopyNew()
    ev.MulThenAdd(a2, 2, acc)
    _check(rg, acc, x + 2 * z, nz.add(na, nz.mulc(na2, 2, float("inf"))), "MulThenAdd integer")
    acc = a.CopyNew()
    ev.MulThenAdd(a2, v, acc)
    _check(rg, acc, x + z * v, nz.add(na, nz.mul(na2, nz.plain(qt))), "MulThenAdd vector")
    acc = new()
    ev.Mul(a, ptw, acc)
    ev.MulThenAdd(a2, ptw, acc)
    _check(rg, acc, x * w + z * w, nz.add(nz.mul(na, nw), nz.mul(na2, nw)), "MulThenAdd pt")
    acc = new(2)
    ev.Mul(a, a2, acc)
    ev.MulThenAdd(a2, a, acc)
    _check(rg, acc, 2 * x * z, nz.add(tm, tm), "MulThenAdd ct")
    acc = new()
    ev.Mul(a, ptw, acc)
    ev.MulRelinThenAdd(a, a2, acc)
    _check(rg, acc, x * w + x * z, nz.rounded(nz.add(nz.mul(na, nw), tm), S * S), "MulRelinThenAdd")
    acc = a.CopyNew()
    ev.MulRelinThenAdd(b, a2, acc)  # the accumulator is scaled up by the integer 3 S
    assert acc.Scale.fraction() == 3 * S * S
    _check(rg, acc, x + y * z, nz.rounded(nz.add(na, nz.mul(nb, na2)), 3.0 * S * S), "MulRelinThenAdd with a scale-up")
    acc = a.CopyNew()
    with pytest.raises(ValueError, match="opOut must be different"):
        ev.MulThenAdd(acc, a2, acc)
    with pytest.raises(ValueError, match="op0.Scale > opOut.Scale"):
        ev.MulThenAdd(b, 0.5, a.CopyNew())
    # SetScale (Mul by the ratio as a big float, RescaleTo) and Rotate
    f = a.CopyNew()
    ev.SetScale(f, 5 * S / 7)
    assert f.Level() == top - 1 and f.Scale.fraction() == REF.Scale(5 * S / 7).fraction()
    ts = nz.rounded(nz.mulc(na, 5 / 7, qt), 5 * S / 7)
    _check(rg, f, x, (na[0], ts[1] * (7 / 5) ** 2), "SetScale")
    o = new(1, f.Level())
    ev.Rotate(f, 1, o)
    _check(rg, o, np.roll(x, -1), nz.rounded((na[0], ts[1] * (7 / 5) ** 2), 5 * S / 7), "Rotate")
    # the other key-switching methods on a fresh ciphertext, ScaleUp and DropLevel
    ks_ = lambda t, times=1: (t[0], t[1] + times * nz.rounded((0, 0.0), S)[1])
    o = new()
    ev.Conjugate(a, o)
    _check(rg, o, np.conj(x), ks_(na), "Conjugate")
    outs = {k: new() for k in (1, 3)}
    ev.RotateHoisted(a, [1, 3], outs)
    for k in (1, 3):
        _check(rg, outs[k], np.roll(x, -k), ks_(na), f"RotateHoisted {k}")
    o = new()
    ev.InnerSum(a, 1, 4, o)  # four rotated copies of the message and of the noise, at most four key switches on the way
    _check(rg, o, sum(np.roll(x, -i) for i in range(4)), ks_((4 * na[0], 4 * na[1]), 4), "InnerSum")
    o = new()
    ev.RotateAndAdd(a, 2, 3, o)
    _check(rg, o, sum(np.roll(x, -2 * i) for i in range(3)), ks_((3 * na[0], 3 * na[1]), 4), "RotateAndAdd")
    o = new()
    ev.ApplyEvaluationKey(a, rg["swk"], o)
    _check(rg, o, x, ks_(na), "ApplyEvaluationKey")
    o = new()
    ev.ScaleUp(a, REF.Scale(4.75), o)  # the words times Uint64(4.75) = 4, the scale times 4.75
    assert o.Scale.fraction() == Fraction(S) * Fraction(4.75)
    _check(rg, o, x * 4 / 4.75, na, "ScaleUp")
    o = a.CopyNew()
    ev.DropLevel(o, 2)
    assert o.Level() == top - 2
    _check(rg, o, x, na, "DropLevel")


@pytest.mark.parametrize("sub", [False, True])
def test_nine_scale_matching_branches_decrypt_to_the_aligned_sum(hostrig, sub):
    """opOut is op0, is op1 or is neither, times op0's scale greater, smaller or equal: the scale-aligned sum, the larger scale"""
    rg = hostrig
    ev, S, nz, rng, N = rg["ev"], rg["S"], rg["noise"], rg["rng"], rg["N"]
    top, seen = len(rg["q"]) - 1, set()
    for s0, s1 in ((5 * S, S), (S, 5 * S), (S, S)):
        for target in ("op0", "op1", "new"):
            x, y = (rng.uniform(-1, 1, N // 2) + 1j * rng.uniform(-1, 1, N // 2) for _ in range(2))
            a, b = _fresh(rg, x, s0), _fresh(rg, y, s1)
            out = {"op0": a, "op1": b, "new": ev.NewCiphertext(1, top)}[target]
            (ev.Sub if sub else ev.Add)(a, b, out)
            seen.add(ev.branch)
            assert out.Scale.fraction() == max(s0, s1)
            _check(rg, out, x - y if sub else x + y, nz.add(nz.fresh(s0), nz.fresh(s1)), (s0 // S, s1 // S, target))
    assert seen == {(w, c) for w in ("op0", "op1", "new") for c in (1, -1, 0)}
