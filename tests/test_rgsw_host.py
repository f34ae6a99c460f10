"""CPU-side tests of the RGSW external product: the restatement of core/rgsw/evaluator.go (tests/rgsw_ref.py) against the
compositions the device routes are built from, against the scheme (decrypt and compare), and the boundary's host mirrors."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O
from tests import boundary as Bd
from tests import rgsw_edges as E
from tests import rgsw_ref as R
from tests.helpers import prod, rng_for, uniform_poly
from tests.rlwe_fixtures import (SecretKey, bfv_encrypt, gen_evaluation_key, gen_evaluation_key_base2, negacyclic_mul_mod, phase,
                                 small_to_rns)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 64
LOG_NTH = 7


def _rings(logq, logp):
    q, p = O.GenModuli(LOG_NTH, list(logq), list(logp))
    return O.Ring(N, q), (O.Ring(N, p) if p else None)


def _ct(rng, ringQ):
    return np.stack([uniform_poly(rng, ringQ.moduli, N) for _ in range(2)])


def _composition(oev, ct, rgsw):
    """ModDown(GadgetProductLazy(ct[0], rgsw[0]) + GadgetProductLazy(ct[1], rgsw[1])), the sum mod q on canonical words"""
    ringQ, ringP = oev.ringQ, oev.ringP
    levelQ, levelP = rgsw[0].LevelQ(), rgsw[0].LevelP()
    aQ, aP = oev.GadgetProductLazy(levelQ, ct[0], rgsw[0])
    bQ, bP = oev.GadgetProductLazy(levelQ, ct[1], rgsw[1])
    sQ = np.stack([ringQ.binop("Add", ringQ.unop("Reduce", aQ[c]), ringQ.unop("Reduce", bQ[c])) for c in range(2)])
    if levelP < 0:
        return sQ
    sP = np.stack([ringP.binop("Add", ringP.unop("Reduce", aP[c]), ringP.unop("Reduce", bP[c])) for c in range(2)])
    return oev.ModDown(levelQ, levelP, sQ, sP)


@pytest.mark.parametrize("pw2", [7, 13])
def test_branch_b_is_the_sum_of_two_gadget_products(pw2):
    ringQ, ringP = _rings((35, 20), (61,))
    rng = rng_for(7100 + pw2)
    oev = O.Evaluator(ringQ, ringP)
    rgsw = R.uniform_rgsw(rng, ringQ, ringP, pw2)
    ct = _ct(rng, ringQ)
    assert np.array_equal(R.external_product(oev, ct, rgsw), _composition(oev, ct, rgsw))


def test_branch_b_without_special_primes():
    ringQ, _ = _rings((35, 20), ())
    rng = rng_for(7120)
    oev = O.Evaluator(ringQ, None)
    rgsw = R.uniform_rgsw(rng, ringQ, None, 7)
    ct = _ct(rng, ringQ)
    assert np.array_equal(R.external_product(oev, ct, rgsw), _composition(oev, ct, rgsw))


def _small_q(bits):
    if bits == 27:
        return 0x7FFF801
    if bits == 14:
        return 0x3001
    return O.GenModuli(LOG_NTH, [bits], [])[0][0]


@pytest.mark.parametrize("bits,pw2", [(27, 7), (14, 7), (28, 4)])
def test_branch_s_equals_branch_b_where_the_sum_cannot_wrap(bits, pw2):
    ringQ = O.Ring(N, [_small_q(bits)])
    rng = rng_for(7130 + bits)
    oev = O.Evaluator(ringQ, None)
    rgsw = R.uniform_rgsw(rng, ringQ, None, pw2)
    ct = _ct(rng, ringQ)
    assert R.takes_32bit_branch(ringQ, rgsw) and R.wrap_bound_holds(ringQ, rgsw)
    assert np.array_equal(R.external_product(oev, ct, rgsw), R.external_product(oev, ct, rgsw, force_bit_decomp=True))


def test_wrap_bound_fails_just_below_2_pow_29():
    q = O.GenModuli(LOG_NTH, [29], [])[0][0]
    while q >> 29:  # a 29-bit-class prime BELOW 2^29 (GenModuli's candidates start above the power of two)
        q -= 2 * N
        while not O.IsPrime(q):
            q -= 2 * N
    ringQ = O.Ring(N, [q])
    rgsw = R.uniform_rgsw(rng_for(7140), ringQ, None, 4)
    assert R.takes_32bit_branch(ringQ, rgsw) and not R.wrap_bound_holds(ringQ, rgsw)


def test_branch_m_is_the_sum_of_two_gadget_products():
    ringQ, ringP = _rings((35, 20), (61, 61))
    rng = rng_for(7150)
    oev = O.Evaluator(ringQ, ringP)
    rgsw = R.uniform_rgsw(rng, ringQ, ringP, 0)
    ct = _ct(rng, ringQ)
    assert np.array_equal(R.external_product(oev, ct, rgsw), _composition(oev, ct, rgsw))


# ---- the scheme: Dec(ExternalProduct(Enc(m0), RGSW(m1))) = m0 m1 up to noise ---------------------------------------------------
SIGMA, EBOUND = 3.2, 19  # the fixtures' error: rounded Gaussian clipped at 19


def _rgsw_encrypt(rng, ringQ, ringP, sk, m1_vals, pw2):
    """rgsw.Encryptor.Encrypt (core/rgsw/encryptor.go): two gadget encryptions of zero with P w m1 added to component 0 of the
    first and to component 1 of the second (the fixtures' keys with skIn = 0 are the encryptions of zero)."""
    zero = np.zeros((len(ringQ.moduli), ringQ.N), dtype=np.uint64)
    LQ, LP = len(ringQ.moduli), (len(ringP.moduli) if ringP is not None else 0)
    P = prod(ringP.moduli) if LP else 1
    m1 = ringQ.unop("MForm", ringQ.NTT(small_to_rns(m1_vals, ringQ.moduli)))
    out = []
    for c in range(2):
        if pw2:
            k = gen_evaluation_key_base2(rng, ringQ, ringP, zero, sk, pw2, SIGMA)
            blk = 0
            for i in range(LQ):
                for j in range(k.nj[i]):
                    g = ringQ.MulScalarBigint(m1, P << (j * pw2))
                    k.q[blk, c, i] = ringQ.binop("Add", k.q[blk, c], g)[i]
                    blk += 1
        else:
            k = gen_evaluation_key(rng, ringQ, ringP, zero, sk, SIGMA)
            g = ringQ.MulScalarBigint(m1, P)
            for d in range(k.q.shape[0]):
                lo, hi = d * LP, min((d + 1) * LP, LQ)
                k.q[d, c, lo:hi] = ringQ.binop("Add", k.q[d, c], g)[lo:hi]
        out.append(O.EvaluationKey(k.q, k.p, pw2=k.pw2, nj=k.nj if pw2 else None))
    return out


def _centred_phase(ringQ, ct, sk):
    Q = prod(ringQ.moduli)
    ph = ringQ.INTT(phase(ringQ, ct, sk.Q))
    w = [(Q // int(qi)) * pow(Q // int(qi), -1, int(qi)) for qi in ringQ.moduli]
    out = []
    for j in range(ringQ.N):
        x = sum(int(ph[i, j]) * w[i] for i in range(len(w))) % Q
        out.append(x - Q if x > Q // 2 else x)
    return out


@pytest.mark.parametrize("logq,logp,pw2", [((35, 20), (61, 61), 0), ((35, 20), (61,), 7), ((35, 20), (61,), 0), ((35, 20), (), 7)],
                         ids=["M", "B-pw2-7", "B-all-ones", "B-no-P"])
def test_external_product_decrypts_to_the_product(logq, logp, pw2):
    ringQ, ringP = _rings(logq, logp)
    rng = rng_for(7200 + 10 * len(logp) + pw2)
    oev = O.Evaluator(ringQ, ringP)
    sk = SecretKey(rng, ringQ, ringP)
    t = 17
    m0 = rng.integers(0, t, size=N)
    m1 = np.zeros(N, dtype=np.int64)
    m1[[3, 17, 40]] = [1, -1, 1]  # a sparse ternary polynomial: ||m1||_1 = 3
    ct = bfv_encrypt(rng, ringQ, sk, m0, t, SIGMA)
    rgsw = _rgsw_encrypt(rng, ringQ, ringP, sk, m1, pw2)
    out = R.external_product(oev, ct, rgsw)
    Q = prod(ringQ.moduli)
    P = prod(ringP.moduli) if ringP is not None else 1
    delta = Q // t
    want = negacyclic_mul_mod(m0, m1 % t, t)
    got = _centred_phase(ringQ, out, sk)
    # the noise, coefficient-wise and worst case: (a) the ciphertext's own error through m1: ||m1||_1 EBOUND, and the part of
    # delta m0 m1 that the reduction of m0 m1 mod t moves: (Q mod t) ||m1||_1; (b) per component and digit, a negacyclic
    # product of a digit (below D_max) with an error polynomial (below EBOUND): N D_max EBOUND, over both components' digits,
    # divided by P; (c) ModDown's rounding of both components against the ternary secret: (1 + N) / 2 each way -> 1 + N
    if pw2:
        digits, dmax = sum(rgsw[0].nj[: len(ringQ.moduli)]), 1 << pw2
    elif len(logp) == 1:
        digits, dmax = len(ringQ.moduli), max(ringQ.moduli)
    else:
        LP = len(logp)
        digits = O.BaseRNSDecompositionVectorSize(len(logq) - 1, LP - 1)
        dmax = max(prod(ringQ.moduli[d * LP:(d + 1) * LP]) for d in range(digits))
    bound = 3 * EBOUND + 3 * (Q % t) + (2 * digits * N * dmax * EBOUND) // P + 1 + (1 + N)
    assert bound < delta // 2, "the shape leaves no room to decrypt"
    worst = 0
    for j in range(N):
        e = got[j] - delta * int(want[j])
        e = (e + Q // 2) % Q - Q // 2
        worst = max(worst, abs(e))
    print(f"noise {worst} (log2 {np.log2(max(worst, 1)):.1f}), bound {bound} (log2 {np.log2(bound):.1f})")
    assert worst <= bound


# ---- the helpers of :283-356 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logp,pw2", [((61,), 7), ((), 7), ((61, 61), 0)])
def test_helpers_build_and_rotate_an_rgsw_encryption(logp, pw2):
    """Encrypt is AddLazy of the gadget plaintext onto encryptions of zero (core/rgsw/encryptor.go); multiplying every row by
    X^alpha - 1 and reducing gives an RGSW encryption of m1 (X^alpha - 1): the external product decrypts to m0 m1 (X^alpha - 1)"""
    ringQ, ringP = _rings((35, 20), logp)
    oev = O.Evaluator(ringQ, ringP)
    seed = 7400 + pw2 + len(logp)
    sk = SecretKey(rng_for(seed), ringQ, ringP)
    m1 = np.zeros(N, dtype=np.int64)
    m1[[3, 17, 40]] = [1, -1, 1]
    want_keys = _rgsw_encrypt(rng_for(seed + 1), ringQ, ringP, sk, m1, pw2)
    zero_keys = _rgsw_encrypt(rng_for(seed + 1), ringQ, ringP, sk, np.zeros(N, dtype=np.int64), pw2)
    P = prod(ringP.moduli) if ringP is not None else 1
    m1ntt = ringQ.unop("MForm", ringQ.NTT(small_to_rns(m1, ringQ.moduli)))
    windows = max(zero_keys[0].nj[:2]) if pw2 else 1
    pt = np.stack([ringQ.MulScalarBigint(m1ntt, P << (j * pw2)) for j in range(windows)])
    built = R.reduce(ringQ, ringP, R.add_lazy_plaintext(ringQ, ringP, pt, zero_keys), zero_keys)
    for k in range(2):
        assert np.array_equal(built[k].q, want_keys[k].q) and np.array_equal(built[k].p, want_keys[k].p)
    alpha = 5
    xQ = R.xpow_alpha_minus_one(ringQ, alpha)
    xP = R.xpow_alpha_minus_one(ringP, alpha) if ringP is not None else None
    rot = R.reduce(ringQ, ringP, R.mul_by_xpow_alpha_minus_one_lazy(ringQ, ringP, built, xQ, xP, built), built)
    m1rot = np.roll(m1, alpha)
    m1rot[:alpha] *= -1
    m1rot = m1rot - m1
    rng = rng_for(seed + 2)
    direct = _rgsw_encrypt(rng, ringQ, ringP, sk, m1rot, pw2)
    t = 17
    m0 = rng.integers(0, t, size=N)
    ct = bfv_encrypt(rng, ringQ, sk, m0, t, SIGMA)
    Q = prod(ringQ.moduli)
    a = _centred_phase(ringQ, R.external_product(oev, ct, rot), sk)
    b = _centred_phase(ringQ, R.external_product(oev, ct, direct), sk)
    delta = Q // t
    want = negacyclic_mul_mod(m0, m1rot % t, t)
    # both decrypt to m0 m1 (X^alpha - 1): the rotated key carries twice the key noise of a fresh one (X^alpha - 1 has norm 2),
    # well inside delta / 2 at these shapes (the bound of the test above, doubled, is below 2^23 against delta > 2^50)
    for got in (a, b):
        for j in range(N):
            e = (got[j] - delta * int(want[j]) + Q // 2) % Q - Q // 2
            assert abs(e) < delta // 4, (j, e)


# ---- the wire format -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logp,pw2", [((61,), 7), ((), 7), ((61, 61), 0)])
def test_wire_is_two_gadget_ciphertexts_back_to_back(logp, pw2):
    """rgsw.Ciphertext.WriteTo / ReadFrom (core/rgsw/elements.go:52-95)"""
    from lattigo_amd import wire
    ringQ, ringP = _rings((35, 20), logp)
    rgsw = R.uniform_rgsw(rng_for(7300 + pw2), ringQ, ringP, pw2)
    parts = [(k.q, k.p, k.pw2, k.nj if pw2 else None) for k in rgsw]
    buf = wire.rgsw_ciphertext_marshal(*parts)
    one = [wire.gadget_ciphertext_marshal(*p) for p in parts]
    assert buf == one[0] + one[1]
    nj = rgsw[0].nj if pw2 else [1] * rgsw[0].q.shape[0]
    assert len(buf) == 2 * wire.gadget_ciphertext_binary_size(nj, 2, len(logp), N)
    back = wire.rgsw_ciphertext_unmarshal(buf)
    for k in range(2):
        kq, kp, b2, njk = back[k]
        assert np.array_equal(kq, rgsw[k].q) and b2 == pw2 and list(njk) == list(nj)
        assert kp.shape[2] == len(logp) and (not logp or np.array_equal(kp, rgsw[k].p))
    with pytest.raises(ValueError):
        wire.rgsw_ciphertext_unmarshal(buf + b"\0")
    with pytest.raises(ValueError):
        wire.rgsw_ciphertext_unmarshal(buf[:-8])


# ---- the constructions of tests/test_gpu_rgsw_edges.py: each has the property it is built for --------------------------------------
def _oracle(s):
    N = 1 << s["logN"]
    oQ, oP = O.Ring(N, s["q"]), (O.Ring(N, s["p"]) if s["p"] else None)
    return N, oQ, oP, O.Evaluator(oQ, oP)


@pytest.mark.parametrize("name", sorted(E.lift_shapes()))
def test_planted_keys_put_the_lift_boundary_into_the_p_accumulator(name):
    s = E.lift_shapes()[name]
    N, oQ, oP, oev = _oracle(s)
    p = s["p"][0]
    if "below-q" in name:
        assert all(p < q for q in s["q"])
    if "between" in name:
        assert min(s["q"]) < p < max(s["q"])
    if "p61" in name:
        assert p == Bd.primes_below(61, s["logN"] + 1, 1)[0]
    ct = np.stack([R.ntt_of_one(oQ, len(s["q"])), np.zeros((len(s["q"]), N), dtype=np.uint64)])
    for component in range(2):
        keys = R.planted_rgsw(rng_for(7500 + component), oQ, oP, s["pw2"], component)
        out, pc = R.external_product(oev, ct, keys, with_p_coeffs=True)
        assert not pc[1 - component].any()
        seen = {int(v) for v in pc[component, 0]}
        assert seen == {(p - 1) // 2, (p + 1) // 2, 0, p - 1}, "a planted residue does not occur"
        assert [int(v) for v in pc[component, 0, :4]] == [(p - 1) // 2, (p + 1) // 2, 0, p - 1]
        # the lift decides the product: with the boundary moved by one ((p - 1) / 2 lifted to (p - 1) / 2 - p) words change
        be = O.BasisExtender(oQ, oP)
        zero = np.zeros_like(out[component])
        shifted = pc[component].copy()
        shifted[0, 0] = (p + 1) // 2
        a = be.ModDownQPtoQNTT(len(s["q"]) - 1, 0, zero, oP.NTT(pc[component]))
        b = be.ModDownQPtoQNTT(len(s["q"]) - 1, 0, zero, oP.NTT(shifted))
        assert not np.array_equal(a, b)


@pytest.mark.parametrize("name", sorted(E.lift_shapes()))
def test_reference_lift_follows_its_float_quotient(name):
    """ModUpPtoQ of one residue (ring/basis_extension.go:195-210 around ModUpExact, :282-308): x = v + (p - 1) / 2 mod p,
    w = uint64(float64(x) / float64(p)), lift = x - w p - (p - 1) / 2.  Below 2^53 that is v > (p - 1) / 2 ? v - p : v; for the
    61-bit prime float64(x) rounds to float64(p) within 128 of p, so (p - 1) / 2 itself and its neighbours below it are lifted to
    v - p: the planted residue (p - 1) / 2 tells the two apart."""
    s = E.lift_shapes()[name]
    N, oQ, oP, _ = _oracle(s)
    p, half = s["p"][0], (s["p"][0] - 1) // 2
    v = R.lift_targets(p, N)
    v[4:12] = [(half - k) % p for k in (1, 2, 64, 127, 128, 129, 300, 1 << 20)]
    got = O.BasisExtender(oQ, oP).ModUpPtoQ(0, len(s["q"]) - 1, v[None])
    w = [int(float((int(x) + half) % p) / float(p)) for x in v]
    for i, q in enumerate(s["q"]):
        assert [int(x) for x in got[i]] == [((int(x) + half) % p - wi * p - half) % q for x, wi in zip(v, w)]
    plain = [int(int(x) > half) for x in v]
    if "p61" in name:
        assert w[0] == 1 and plain[0] == 0 and w[1:4] == [0, 0, 0] and w[4:8] == [1, 1, 1, 1] and w[10:12] == [0, 0]
    else:
        assert not any(w)


@pytest.mark.parametrize("pw2", [7, 13, 14])
def test_all_mask_coefficients_have_every_window_equal_to_the_mask(pw2):
    mask = (1 << pw2) - 1
    for q in Bd.class_chain(9, "hiIdD") + [E.Q14]:
        c = R.all_mask_coeffs(q, pw2, 8)
        nj = R.window_counts([q], pw2)[0]
        w = [int(R.mask_vec(c, j * pw2, mask)[0]) for j in range(nj)]
        assert int(c[0]) < q and all(x == mask for x in w[:-1]) and w[-1] == (q >> ((nj - 1) * pw2)) - 1
    mods = [E.Q14, Bd.primes_below(47, 10, 1)[0]]
    assert [int(v) for v in E.coeffs("coeff_max", mods, 4, pw2)[:, 0]] == [m - 1 for m in mods]
    assert not E.coeffs("coeff_zero", mods, 4, pw2).any()
    # the cycle of ciphertext words reaches every kind in ten polynomials, lazy words up to 2q - 1 included
    ring = O.Ring(64, O.GenModuli(LOG_NTH, [35, 20], [])[0])
    cyc = E.CtCycle(ring, pw2, start=5)
    polys = [cyc(rng_for(7600), ring.moduli, 64) for _ in range(10)]
    assert max(int(x[0].max()) for x in polys) == 2 * int(ring.moduli[0]) - 1
    want = ring.NTT(E.coeffs("coeff_mask", ring.moduli, 64, pw2))
    assert any(np.array_equal(x, want) for x in polys) and any(not x.any() for x in polys)


def test_digit_index_shapes():
    sh = E.digit_index_shapes()
    nj = {k: R.window_counts(v["q"], 1) for k, v in sh.items()}
    assert sum(nj["beta255"]) == 255 and E.fused_by_header(9, len(sh["beta255"]["q"]), 0)
    assert sum(nj["prefix255"][:-1]) == 255 and sum(nj["prefix256"][:-1]) >= 256   # prefix[levelQ]
    assert all(E.fused_by_header(9, len(sh[k]["q"]), 0) for k in ("prefix255", "prefix256"))
    for v in sh.values():
        assert len(set(v["q"])) == len(v["q"]) and all(O.IsPrime(q) and q % 1024 == 1 for q in v["q"])


def test_shift_and_domain_shapes_lie_where_the_header_says():
    for s in E.shift_shapes().values():
        last = (s["nj"][0] - 1) * s["pw2"]
        assert last in (63, 64) and (last < 64) == (s["route"] == E.ONE) and s["nj"][0] * s["pw2"] <= 64 + s["pw2"]
    dom = E.domain_shapes()
    for s in dom.values():
        assert (s["route"] == E.ONE) == E.fused_by_header(s["logN"], len(s["q"]), len(s["p"]))
    assert [len(dom[k]["q"]) for k in ("9x7+P", "9x8+P", "10x3+P", "10x3", "10x4+P", "11x1+P", "11x2+P")] == [7, 8, 3, 3, 4, 1, 2]
    assert dom["9x8+P"]["q"][:7] == dom["9x7+P"]["q"] and dom["10x4+P"]["q"][:3] == dom["10x3+P"]["q"]
    for name, s in E.moduli_shapes().items():
        assert (s["route"] == E.ONE) == (E.fused_by_header(s["logN"], len(s["q"]), len(s["p"])))
        assert len(set(s["q"] + s["p"])) == len(s["q"] + s["p"])
    m = E.moduli_shapes()
    assert {Bd.modulus_class(q) for q in m["12-dihDI|i"]["q"]} == {0, 1, 2} and len(m["12-dihd|ih"]["p"]) == 2
    big = [q for q in m["9-hiIdD+14|h-pw2-14"]["q"] + m["9-hiIdD+14|h-pw2-14"]["p"] if q <= (1 << 14) - 1]
    assert big == [E.Q14] and E.Q14 > (1 << 13) - 1


@pytest.mark.parametrize("name", ["9-hiIdD+14|h-pw2-16", "9-hiIdD+14|h-all-ones"])
def test_windows_exceed_the_transform_input_bound_of_one_destination(name):
    """the forward transform of the one-launch kernel takes words below 4q: with a 16-bit mask (and with the all-ones mask) the
    windows of the worst-case coefficients reach 4 * 12289 and beyond, so the 14-bit destination depends on the reduction before
    the transform; the 16-bit mask stays below every other modulus of the chain"""
    s = E.moduli_shapes()[name]
    mask = (1 << s["pw2"]) - 1 if s["pw2"] else (1 << 64) - 1
    assert mask >= 4 * E.Q14
    if s["pw2"]:
        assert [mask >= m for m in s["q"] + s["p"]].count(True) == 1 and all(mask < m for m in s["q"] + s["p"] if m != E.Q14)
    nj = R.window_counts(s["q"], s["pw2"]) if s["pw2"] else [1] * len(s["q"])
    for kind in ("coeff_max", "coeff_mask"):
        c = E.coeffs(kind, s["q"], 4, s["pw2"])
        w = [int(R.mask_vec(c[i], j * s["pw2"], mask)[0]) for i in range(len(s["q"])) for j in range(nj[i])]
        assert sum(x >= 4 * E.Q14 for x in w) >= 4, (kind, w)   # (several source limbs have such a window)
        assert s["pw2"] or max(w) >> 60 == 1                     # (all-ones: a whole 61-bit coefficient)


@pytest.mark.parametrize("pw2", range(1, 9))
def test_wrap_bound_sides(pw2):
    lo, hi = E.wrap_primes()
    assert lo < hi < (1 << 29) and (1 << 28) < lo and all(O.IsPrime(q) and q % 2048 == 1 for q in (lo, hi))
    for side, q in enumerate((lo, hi)):
        ringQ = O.Ring(1024, [q])
        keys = R.uniform_rgsw(rng_for(7700), ringQ, None, pw2)
        assert R.takes_32bit_branch(ringQ, keys) and keys[0].q.shape[0] == (29 + pw2 - 1) // pw2
        assert R.wrap_bound_holds(ringQ, keys) == (pw2 >= 4 or (pw2 == 3 and side == 0)), (q, pw2)


def test_key_words_domain_and_lazy_keys_on_the_oracle():
    """hering_rgsw.h, "Key words": inside the bound the reference's product with a key after AddLazy is the product with the
    reduced key (its Montgomery products stay exact); a 61-bit modulus leaves no room for M = 2"""
    for logq, logp, pw2 in (((35, 20), (55,), 7), ((35, 20), (55, 60), 0), ((27,), (), 7)):
        ringQ, ringP = _rings(logq, logp)
        oev = O.Evaluator(ringQ, ringP)
        rng = rng_for(7800 + pw2 + len(logp))
        a, b = R.uniform_rgsw(rng, ringQ, ringP, pw2), R.uniform_rgsw(rng, ringQ, ringP, pw2)
        lazy = R.add_lazy_ciphertext(ringQ, ringP, a, b)
        assert any(int(k.q[:, :, 0].max()) >= ringQ.moduli[0] for k in lazy)
        assert R.key_words_in_domain(ringQ, ringP, lazy, 2)
        ct = _ct(rng, ringQ)
        assert np.array_equal(R.external_product(oev, ct, lazy), R.external_product(oev, ct, R.reduce(ringQ, ringP, lazy, lazy)))
    ringQ, ringP = _rings((35, 20), (61,))
    keys = R.uniform_rgsw(rng_for(7810), ringQ, ringP, 7)
    assert R.key_words_in_domain(ringQ, ringP, keys, 1) and not R.key_words_in_domain(ringQ, ringP, keys, 2)
    p = int(ringP.moduli[0])
    assert (2 * p - 1) * (6 * p - 2) >= (p << 64)


# ---- the boundary's host side --------------------------------------------------------------------------------------------
def test_header_symbols_exported():
    import __graft_entry__ as graft
    from lattigo_amd import _lib
    graft.build()
    L = _lib.load()
    want = ["he_rgsw_external_product", "he_rgsw_keyset_create", "he_rgsw_keyset_destroy", "he_rgsw_external_product_select"]
    syms = _lib.declared_symbols()
    assert all(s in syms for s in want), "include/hering_rgsw.h is not among the declared headers"
    assert all(hasattr(L, s) for s in want)


def test_aliasing_rows_hold_against_the_header():
    """tests/rgsw_aliasing.py names the polynomial parameters of the two product entries as include/hering_rgsw.h declares them,
    in header order, and allows exactly the reference's op0 == opOut"""
    import re
    from tests import rgsw_aliasing as RA
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hering_rgsw.h")).read(), flags=re.S)
    for name, row in RA.ROWS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m, name
        params = [p.split()[-1].lstrip("*") for p in m.group(1).split(",")]
        assert [p for p in params if p in row.params] == list(row.params), (name, params)
        assert row.allowed == {("out0", "in0"), ("out1", "in1")}
        assert row.verdict("in0", "in1") == "accept" and row.verdict("out0", "out1") == "reject"
        assert row.verdict("out0", "in1") == "reject" and row.verdict("out1", "in0") == "reject"


def test_go_shim_defines_external_product():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_go_abi.py")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ExternalProduct" in out.stdout


def test_cpp_mirror_compiles(tmp_path):
    """include/hering.hpp's rgsw::Ciphertext / rgsw::Evaluator::ExternalProduct type-check against hering_rgsw.h"""
    src = tmp_path / "rgsw_mirror.cpp"
    src.write_text(
        '#include "hering.hpp"\n'
        "void f(hering::rgsw::Evaluator &ev, hering::Ciphertext &op0, hering::rgsw::Ciphertext &op1, hering::Ciphertext &out) {\n"
        "    ev.ExternalProduct(op0, op1, out);\n"
        "    (void)op1.LevelQ(); (void)op1.LevelP();\n"
        "}\n")
    out = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
