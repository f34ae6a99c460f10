"""The cases the RGSW-encryptor tests share: shapes (the chains of tests/keygen_cases.py and the blind-rotation shapes of
tests/test_gpu_blindrot.py), seeds, plaintexts and the restatement's result for each (tests/rgsw_encryptor_ref.py), computed once.
tests/test_rgsw_encryptor_host.py runs every case three times -- as is, with exp / log moved 4 ulps up and 4 ulps down -- and asks
for identical words and positions, the rule of tests/keygen_cases.py: a case that fails gets another seed, never a looser
comparison."""
from __future__ import annotations

import functools
import math

import numpy as np

from oracle import oracle as O
from tests import keygen_cases as K
from tests import keygen_ref as KR
from tests import rgsw_edges as E
from tests import rgsw_encryptor_ref as GR
from tests import sampler_ref as R

SIGMA, BOUND = K.SIGMA, K.BOUND
Q27 = 0x7FFF801  # the reference's blind rotation modulus (blindrot_test.go:55)
Q_LWE, N_LWE = 0x3001, 16

C_BR_Q27 = K._case("blindrot-9-q27-pw2-7", 9, [Q27], (), 601, pw2=7)
C_BR_P61 = K._case("blindrot-9-35-20-P61-pw2-7", 9, *E.moduli(9, (35, 20), (61,)), 602, pw2=7)
# 2 + 0 limbs (no special prime, window counts differing per limb), 2 + 1 with pw2 7, the partial last digit, a key below the top
# levels, the rejecting modulus, the class boundary, a conjugate-invariant ring, the two-launch transform, the blind-rotation shapes
CASES = [K.C_B16_NOP, K.C_B7, K.C_3P2, K.C_LOW, K.C_REJECT, K.C_CLASS, K.C_CI, K.C_BIG, C_BR_Q27, C_BR_P61]
FORMS_CASE = K.C_3P2
TABLE_CASE = K.C_B7
TABLE_SEL, TABLE_M = [1, -1, 0, 1, 2], 3
REJECT_TABLE_SEL = [0, -1]
COMPOSED_CASES = [K.C_3P2, K.C_B16_NOP]
ORDER_CASE = K.C_LOW
E2E_CASE = C_BR_Q27


def encryptor(c: K.Case, seed, exp=math.exp, log=R._log):
    oQ, oP = K.rings(c)
    src = R.seeded_source(seed)
    return GR.Encryptor(oQ, oP, src, K.secret(c), SIGMA, BOUND, exp, log), src


def plaintext(c: K.Case, salt=0):
    """[limbs of Q][N] canonical uniform words, nonzero in every limb"""
    return K.uniform_poly(c, 40 + salt)


def run_encrypt(c: K.Case, form=(True, True), exp=math.exp, log=R._log):
    """(ciphertext, its Gaussians [u][row], the position of the source afterwards); form = (pt_is_ntt, pt_is_montgomery)"""
    enc, src = encryptor(c, c.seed + 1000, exp, log)
    ct = enc.encrypt(plaintext(c), form[0], form[1], c.levelQ, c.levelP, c.pw2)
    return ct, enc.gaussians[0], src.pos


def run_zero(c: K.Case, exp=math.exp, log=R._log):
    enc, src = encryptor(c, c.seed + 1000, exp, log)
    return enc.encrypt_zero(c.levelQ, c.levelP, c.pw2), enc.gaussians[0], src.pos


def table_plaintexts(c: K.Case, m):
    return np.stack([plaintext(c, 1 + s) for s in range(m)])


def run_table(c: K.Case, sel, m, exp=math.exp, log=R._log):
    """(ciphertexts, Gaussians per ciphertext, position)"""
    enc, src = encryptor(c, c.seed + 2000, exp, log)
    return enc.encrypt_table(table_plaintexts(c, m), sel, c.levelQ, c.levelP, c.pw2), enc.gaussians, src.pos


# ---- blindrot.GenEvaluationKeyNew at the parameters of test_evaluate_end_to_end ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lwe_ring():
    return O.Ring(N_LWE, [Q_LWE])


@functools.lru_cache(maxsize=None)
def lwe_secret():
    """sk.Value.Q of the LWE ring, from a source of its own (the density sampler walks bits: no exp / log)"""
    return KR.KeyGenerator(lwe_ring(), None, R.seeded_source(E2E_CASE.seed + 7000), K.XS_P, SIGMA, BOUND).gen_secret_key(0, -1)[0]


def run_blindrot(one_source: bool, exp=math.exp, log=R._log):
    """(RGSW ciphertexts, {Galois element: key}, Gaussians, (position of the encryptor's source, of the generator's))"""
    c = E2E_CASE
    oQ, oP = K.rings(c)
    src = R.seeded_source(c.seed + 3000)
    src_kg = None if one_source else R.seeded_source(c.seed + 3001)
    brk, gks, g_rgsw, g_gal = GR.gen_evaluation_key_new(oQ, oP, K.secret(c), lwe_ring(), lwe_secret(), c.levelQ, c.levelP, c.pw2, src, src_kg,
                                                        SIGMA, BOUND, exp, log)
    return brk, gks, (g_rgsw, g_gal), (src.pos, None if one_source else src_kg.pos)


want_encrypt = functools.lru_cache(maxsize=None)(lambda c, form=(True, True): run_encrypt(c, form))
want_zero = functools.lru_cache(maxsize=None)(lambda c: run_zero(c))
want_table = functools.lru_cache(maxsize=None)(lambda c, sel, m: run_table(c, list(sel), m))
want_blindrot = functools.lru_cache(maxsize=None)(lambda one_source: run_blindrot(one_source))


def same_ct(a, b):
    return K.same_key(a[0], b[0]) and K.same_key(a[1], b[1])
