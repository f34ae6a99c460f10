"""blindrot.Evaluator.Evaluate and BlindRotateCore (core/rgsw/blindrot/evaluator.go:49-307) restated on the oracle: the schedule
with the reference's own maps (Python dicts for Go's), the accumulator through oracle.Evaluator.Automorphism and
tests/rgsw_ref.external_product, the prologue on Python integers.  Key material for the semantic tests comes from
tests/rlwe_fixtures.py (our own seeded sampler).

Polynomials are [limbs, N] uint64; a ciphertext is [2, limbs, N]; an RGSW ciphertext a pair of oracle EvaluationKeys."""
from __future__ import annotations

import math

import numpy as np

from oracle import oracle as O
from tests import rgsw_ref as R
from tests import rlwe_fixtures as F
from tests.helpers import div_round, prod

windowSize = 10  # keys.go:14
GaloisGen = 5

AUTO, PROD = "automorphism", "external_product"


def galois_element(N: int, k: int) -> int:
    """Parameters.GaloisElement (core/rlwe/params.go:580), standard ring"""
    return pow(GaloisGen, k & (2 * N - 1), 2 * N)


def galois_elements(N: int):
    """keys.go:94-99"""
    return [galois_element(N, i + 1) for i in range(windowSize)] + [2 * N - GaloisGen]


def galois_element_inverse_map(N: int) -> dict:
    """getGaloisElementInverseMap (:232-255): map[+-g^k mod 2N] = +-k; 2N - 1 gets -0 = 0"""
    twoN, m, pw = N << 1, {}, 1
    for i in range(N >> 1):
        m[pw] = i
        m[twoN - pw] = -i
        pw = pw * GaloisGen & (twoN - 1)
    return m


def discrete_log_sets(N: int, a) -> dict:
    """getDiscreteLogSets (:258-280); a missing key of a Go map reads as 0; a non-zero even word panics"""
    dlog = galois_element_inverse_map(N)
    sets = {}
    for i, ai in enumerate(a):
        ai = int(ai)
        if ai & 1 != 1 and ai != 0:
            raise ValueError("getDiscreteLogSets: a[i] is not odd and thus not an element of Z_{2N}^{*}")
        sets.setdefault(dlog.get(ai, 0), []).append(i)
    return sets


def schedule(N: int, a):
    """BlindRotateCore (:135-186) with evaluateFromDiscreteLogSets (:189-229) as the list of operations on the accumulator"""
    sets = discrete_log_sets(N, a)
    ops = []

    def step(k, v):
        if k in sets:
            if v != 0:
                ops.append((AUTO, galois_element(N, v)))
                v = 0
            for j in sets[k]:
                ops.append((PROD, j))
        v += 1
        if v == windowSize or k == 1:
            ops.append((AUTO, galois_element(N, v)))
            v = 0
        return v

    Nhalf = N >> 1
    v = 0
    for i in range(Nhalf - 1, 0, -1):  # :156
        v = step(-i, v)
    step(N << 1, 0)                    # :163, its result is dropped
    ops.append((AUTO, 2 * N - GaloisGen))  # :169
    for i in range(Nhalf - 1, 0, -1):  # :174
        v = step(i, v)
    step(0, 0)                         # :181
    return ops


def rounds_of(ops) -> int:
    """rounds one list needs on its own: an automorphism and the external product that follows it share a round"""
    n = p = 0
    while p < len(ops):
        if ops[p][0] == AUTO:
            p += 1
        if p < len(ops) and ops[p][0] == PROD:
            p += 1
        n += 1
    return n


def blind_rotate_core(oev: O.Evaluator, a, acc: np.ndarray, brk, gks: dict) -> np.ndarray:
    """acc [2, limbs, N] -> BlindRotateCore(a, acc, BRK); brk: list of RGSW pairs, gks: {Galois element: oracle key}"""
    for kind, arg in schedule(oev.ringQ.N, a):
        acc = oev.Automorphism(acc, arg, gks[arg]) if kind == AUTO else R.external_product(oev, acc, brk[arg])
    return acc


def mod_switch_to_2N(ringQ: O.Ring, pol: np.ndarray, twoN: int, make_odd: bool):
    """modSwitchRLWETo2NLvl (:284-307): pol [limbs, N] coefficient domain -> round(x 2N / Q) & (2N - 1)"""
    moduli = [int(q) for q in ringQ.moduli]
    Q = prod(moduli)
    w = [(Q // q) * pow(Q // q, -1, q) for q in moduli]
    out = []
    for j in range(pol.shape[1]):
        x = sum(int(pol[i, j]) * w[i] for i in range(len(moduli))) % Q
        t = div_round(x * twoN, Q) & (twoN - 1)
        if make_odd and t & 1 == 0 and t != 0:
            t ^= 1
        out.append(t)
    return out


def mul_by_small_monomial_mod_2N(mask: int, pol: list, n: int) -> list:
    """mulBySmallMonomialMod2N (utils.go:11)"""
    if n == 0:
        return pol
    N = len(pol)
    pol = pol[N - n:] + pol[:N - n]
    return [(-x & mask) if j < n else x for j, x in enumerate(pol)]


def rows_and_b(ringQLWE: O.Ring, ct: np.ndarray, NBR: int, slots, is_ntt: bool = True):
    """the prologue of Evaluate (:65-103): ({slot: a row}, {slot: b})"""
    c = np.stack([ringQLWE.INTT(ct[k]) if is_ntt else ct[k] for k in range(2)])
    NLWE = ringQLWE.N
    mask = (NBR << 1) - 1
    tmp1 = mod_switch_to_2N(ringQLWE, c[1], NBR << 1, True)
    a = [tmp1[0]] + [-tmp1[NLWE - j] & mask for j in range(1, NLWE)]
    b = mod_switch_to_2N(ringQLWE, c[0], NBR << 1, False)
    rows, prev = {}, 0
    for index in range(NLWE):
        if index in slots:
            a = mul_by_small_monomial_mod_2N(mask, a, index - prev)
            prev = index
            rows[index] = list(a)
    return rows, {i: b[i] for i in rows}


def monomial(ringQ: O.Ring, i: int) -> np.ndarray:
    """NewMonomialXi (ring/ring.go:374)"""
    N = ringQ.N
    p = np.zeros((len(ringQ.moduli), N), dtype=np.uint64)
    i &= (N << 1) - 1
    for k, q in enumerate(ringQ.moduli):
        if i >= N:
            p[k, i - N] = int(q) - 1
        else:
            p[k, i] = 1
    return p


def init_accumulator(ringQBR: O.Ring, test_poly: np.ndarray, b: int) -> np.ndarray:
    """Acc = (f(X^-g) X^(-g b), 0) (:108-113)"""
    Xb = ringQBR.unop("MForm", ringQBR.NTT(monomial(ringQBR, b)))
    t = ringQBR.binop("MulCoeffsMontgomery", test_poly, Xb)
    return np.stack([ringQBR.AutomorphismNTT(t, 2 * ringQBR.N - GaloisGen), np.zeros_like(t)])


def evaluate(oev: O.Evaluator, ringQLWE: O.Ring, ct: np.ndarray, test_polys: dict, brk, gks: dict, ntt_flag: bool = True,
             is_ntt: bool = True) -> dict:
    """Evaluate (:49-132) -> {slot: [2, limbs, N]}"""
    ringQBR = oev.ringQ
    rows, b = rows_and_b(ringQLWE, ct, ringQBR.N, test_polys, is_ntt)
    res = {}
    for index, a in rows.items():
        acc = blind_rotate_core(oev, a, init_accumulator(ringQBR, test_polys[index], b[index]), brk, gks)
        res[index] = acc if ntt_flag else np.stack([ringQBR.INTT(acc[0]), ringQBR.INTT(acc[1])])
    return res


# ---- InitTestPolynomial (blindrot.go:12) ------------------------------------------------------------------------------------------
def scale_up(value: float, scale: float, Q: int) -> int:
    """scaleUp (utils.go:26)"""
    x = -scale * value if value < 0 else scale * value
    res = int(math.floor(x + 0.5)) % Q
    return Q - res if value < 0 else res


def init_test_polynomial(g, scale: float, ringQ: O.Ring, a: float, b: float) -> np.ndarray:
    N = ringQ.N
    inv = lambda x: (x * (b - a) + b + a) / 2.0
    interval = 2.0 / float(N)
    Fp = np.zeros((len(ringQ.moduli), N), dtype=np.uint64)
    for j, q in enumerate(ringQ.moduli):
        for i in range((N >> 1) + 1):
            Fp[j, i] = scale_up(g(inv(-interval * float(i))), scale, int(q))
        for i in range((N >> 1) + 1, N):
            Fp[j, i] = scale_up(-g(inv(interval * float(N - i))), scale, int(q))
    return ringQ.NTT(Fp)


def sign(x: float) -> float:
    """blindrot_test.go:33-44"""
    return 1.0 if x > 0 else (0.0 if x == 0 else -1.0)


# ---- key material (GenEvaluationKeyNew, keys.go:46-108) with the fixtures' sampler -------------------------------------------------
def rgsw_encrypt(rng, ringQ: O.Ring, ringP, sk: F.SecretKey, m_ntt: np.ndarray, pw2: int):
    """rgsw.Encryptor.Encrypt (core/rgsw/encryptor.go): two gadget encryptions of zero with m times the gadget vector added to
    component 0 of the first and to component 1 of the second; m_ntt: the plaintext in the NTT domain"""
    m = ringQ.unop("MForm", m_ntt)
    zero = np.zeros_like(m)
    k0 = F.gen_evaluation_key_base2(rng, ringQ, ringP, m, sk, pw2)
    k1 = F.gen_evaluation_key_base2(rng, ringQ, ringP, zero, sk, pw2)
    P = prod(ringP.moduli) if ringP is not None else 1
    blk = 0
    for i in range(len(ringQ.moduli)):
        for j in range(k1.nj[i]):
            g = ringQ.MulScalarBigint(m, P << (j * pw2))
            k1.q[blk, 1, i] = ringQ.binop("Add", k1.q[blk, 1], g)[i]
            blk += 1
    return [k0, O.EvaluationKey(k1.q, k1.p, pw2=pw2, nj=k1.nj)]


def gen_blind_rotation_keys(rng, ringQ: O.Ring, ringP, sk: F.SecretKey, sk_lwe_vals, pw2: int):
    """(RGSW(X^s[i]) for every coefficient of the LWE secret, {Galois element: base-2 Galois key})"""
    cache = {}
    brk = []
    for s in sk_lwe_vals:
        s = int(s)
        if s not in cache:
            cache[s] = ringQ.NTT(monomial(ringQ, s))
        brk.append(rgsw_encrypt(rng, ringQ, ringP, sk, cache[s], pw2))
    gks = {}
    for g in galois_elements(ringQ.N):
        ginv = pow(g, 2 * ringQ.N - 1, 2 * ringQ.N)
        gks[g] = F.gen_evaluation_key_base2(rng, ringQ, ringP, sk.Q, F.automorphism_secret(rng, ringQ, ringP, sk, ginv), pw2)
    return brk, gks


def encrypt_lwe_values(rng, ringQ: O.Ring, sk: F.SecretKey, values, scale: float, sigma: float = 3.2) -> np.ndarray:
    """blindrot_test.go:108-124: the values at `scale` in the first coefficients of one RLWE sample, NTT domain"""
    N, q = ringQ.N, int(ringQ.moduli[0])
    pt = np.zeros((1, N), dtype=np.uint64)
    for i, v in enumerate(values):
        pt[0, i] = q - int(-v * scale) if v < 0 else int(v * scale)
    e = np.clip(np.rint(rng.normal(0.0, sigma, size=N)), -19, 19).astype(np.int64)
    c1 = np.stack([rng.integers(0, q, size=N, dtype=np.uint64)])
    m = ringQ.binop("Add", ringQ.NTT(pt), ringQ.NTT(F.small_to_rns(e, ringQ.moduli)))
    return np.stack([ringQ.binop("Sub", m, ringQ.binop("MulCoeffsMontgomery", c1, sk.Q)), c1])


def decode(ringQ: O.Ring, ct: np.ndarray, sk: F.SecretKey, scale: float, is_ntt: bool = True) -> float:
    """blindrot_test.go:141-160: coefficient 0 of the decryption over the scale"""
    if not is_ntt:
        ct = np.stack([ringQ.NTT(ct[0]), ringQ.NTT(ct[1])])
    c = int(ringQ.INTT(F.phase(ringQ, ct, sk.Q))[0, 0])
    q = int(ringQ.moduli[0])
    return -float(q - c) / scale if c >= (q >> 1) else float(c) / scale
