"""The restatement of rlwe.Encryptor / rlwe.Decryptor (tests/encryptor_ref.py) held against what an encryption is, the cases of the
GPU tests (tests/encryptor_cases.py) held against the exp / log condition they rest on, and the header's symbols.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

import __graft_entry__ as graft
from lattigo_amd import _lib
from tests import encryptor_aliasing as A
from tests import encryptor_cases as K
from tests import encryptor_ref as ER
from tests import sampler_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hering_encryptor.h")
ENTRIES = {"he_encrypt_zero", "he_encrypt_zero_qp", "he_add_pt_to_ct", "he_encrypt", "he_decryptor_decrypt"}


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_symbols_exported_and_left_out_of_recordings(lib):
    mine = sorted(set(re.findall(r"\b(he_[a-z0-9_]+)\s*\(", _header())))
    assert len(mine) == 10 and all(s in _lib.declared_symbols() and hasattr(lib, s) for s in mine), mine
    tables = (_lib._TRACE_FNS, _lib._TRACE_FNS_RGSW, _lib._TRACE_FNS_BLINDROT, _lib._TRACE_FNS_BRIDGE, _lib._TRACE_FNS_BFV)
    for s in mine:
        assert not any(s in t for t in tables), s  # no replay numbers
        assert (s in _lib._TRACE_IGNORE) == (s not in ENTRIES), s  # an entry draws from the source: it fails a recording


def test_prototypes_live_in_the_new_header_only():
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h.endswith(".h") and h != "hering_encryptor.h":
            src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
            assert not re.search(r"\bhe_(encrypt|decrypt|add_pt_to_ct)", src), h


def test_aliasing_table_covers_the_header():
    """every entry of the header with a polynomial operand has a row whose parameters are the header's, in order (then `key`); no
    pair with an output in it is allowed"""
    entries = {}
    for m in re.finditer(r"\bint\s+(he_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", _header(), flags=re.S):
        polys = [p.split()[-1].lstrip("*") for p in m.group(2).split(",") if "he_handle" in p.split()[:2] and re.match(r"\*?(c[01][QP]?|pt|ct)$", p.split()[-1])]
        if polys:
            entries[m.group(1)] = polys
    assert sorted(entries) == sorted(A.ROWS) == sorted(ENTRIES)
    for name, polys in entries.items():
        row = A.ROWS[name]
        assert [p for p in row.params if p != "key"] == polys, (name, polys)
        assert not row.allowed
        outs = [p for p in row.params if row.written(p)]
        assert all((a, b) in A.refused_pairs(row) or (b, a) in A.refused_pairs(row) for a in outs for b in row.params if a != b)


# ---- the stream check the GPU tests rest on ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", K.ZERO_CASES + K.GENPK_CASES + K.ENCRYPT_CASES, ids=lambda c: c.id)
def test_no_case_depends_on_exp_or_log(c):
    """every draw of a case is made before any flag is read, so one pair of flags covers the case's Gaussian draws; all three runs
    must agree on every word and on the position"""
    base = K.want_zero(c, 1, 0)
    for ulps in (4, -4):
        assert K.same(base, K.run_zero(c, 1, 0, R.shifted(math.exp, ulps), R.shifted(R._log, ulps))), ulps


def test_the_sequence_of_two_calls_does_not_depend_on_exp_or_log():
    ws, pos = K.run_sequence()
    for ulps in (4, -4):
        ws2, pos2 = K.run_sequence(R.shifted(math.exp, ulps), R.shifted(R._log, ulps))
        assert all(K.same((a, pos), (b, pos2)) for a, b in zip(ws, ws2)), ulps


# ---- what an encryption is -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npp,qp", [(0, False), (1, False), (1, True)])
@pytest.mark.parametrize("is_ntt,is_mont", [(1, 0), (0, 0)])
def test_decrypt_of_encrypt_zero_sk_is_the_gaussian_drawn(npp, qp, is_ntt, is_mont):
    logN, nq = 5, 2
    oQ, oP = K.rings(logN, nq, npp)
    _, skQ, skP = K.ternary_secret(np.random.default_rng(7), oQ, oP)
    enc = ER.Encryptor(oQ, oP, R.seeded_source(41))
    ((c0, _), (c1, _)), = enc.encrypt_zero_sk([(skQ, skP)], nq - 1, 0 if qp else -1, is_ntt, is_mont)
    pt, level = ER.decrypt(oQ, skQ, [c0, c1], nq - 1, nq - 1, is_ntt)
    if is_ntt:
        pt = oQ.INTT(pt)
    e = enc.drawn[0]
    assert level == nq - 1 and all(np.array_equal(pt[i], e[i] % np.uint64(q)) for i, q in enumerate(oQ.moduli))  # (the word q_i itself is 0)
    assert any(K.centered(e[0], oQ.moduli[0]))


@pytest.mark.parametrize("npp", [0, 2])
def test_decrypt_of_encrypt_pk_is_the_message_within_the_noise_drawn(npp):
    """pk = (-a s + e_pk, a).  w = u e_pk + e0 + e1 s over the integers, from the polynomials the restatement drew.  Without P the
    decryption is m + w exactly.  With P it is m + (w + r0 + r1 s) / P, where ModDownQPtoQ rounds each component and differs from
    the exact quotient by at most 1, so every coefficient of the difference is within max|w| / P + 1 + (1 + |s|_1)."""
    logN, nq = 5, 2
    N = 1 << logN
    oQ, oP = K.rings(logN, nq, npp)
    s, skQ, skP = K.ternary_secret(np.random.default_rng(8), oQ, oP)
    src = R.seeded_source(43)
    enc = ER.Encryptor(oQ, oP, src)
    pk, = enc.encrypt_zero_sk([(skQ, skP)], nq - 1, npp - 1, 1, 1)  # GenPublicKey (keygenerator.go:80-88)
    m = np.stack([np.arange(N, dtype=np.uint64) * np.uint64(1 << 20)] * nq)
    if npp:
        ((c0, _), (c1, _)), = enc.encrypt_zero_pk([pk], nq - 1, -1, False, 0, 0)
        c0 = enc.add_pt_to_ct(nq - 1, m, False, c0, False)
        pt, _ = ER.decrypt(oQ, skQ, [c0, c1], nq - 1, nq - 1, 0)
    else:  # (the NTT-domain branch: the one whose Gaussians are read apart from the sum, :322-324)
        ((c0, _), (c1, _)), = enc.encrypt_zero_pk_nop([pk], nq - 1, 1)
        c0 = enc.add_pt_to_ct(nq - 1, oQ.NTT(m), True, c0, True)
        pt = oQ.INTT(ER.decrypt(oQ, skQ, [c0, c1], nq - 1, nq - 1, 1)[0])
    assert len(enc.drawn) == 4
    e_pk, u, e0, e1 = (K.centered(x[0], oQ.moduli[0]) for x in enc.drawn)
    w = [a + b + c for a, b, c in zip(K.negacyclic(u, e_pk), e0, K.negacyclic(e1, [int(x) for x in s]))]
    assert any(w) and src.pos > 0
    for i, q in enumerate(oQ.moduli):
        diff = K.centered([(int(a) - int(b)) % q for a, b in zip(pt[i], m[i])], q)
        if npp:
            Pmod = oP.moduli[0]  # (encryptZeroPk on a ring.Poly element: levelP = 0, :217)
            bound = max(abs(x) for x in w) / Pmod + 1 + 1 + int(np.abs(s).sum())
            assert max(abs(x) for x in diff) <= bound, (i, max(abs(x) for x in diff), bound)
        else:
            assert diff == w, i


def test_add_pt_to_ct_transforms_as_the_reference_writes_it():
    oQ, _ = K.rings(5, 2, 0)
    rng = np.random.default_rng(3)
    pt, c0 = K.uniform(rng, oQ.moduli, 32), K.uniform(rng, oQ.moduli, 32)
    enc = ER.Encryptor(oQ, None, R.seeded_source(1))
    assert np.array_equal(enc.add_pt_to_ct(1, pt, True, c0, False), oQ.binop("Add", c0, oQ.NTT(pt)))  # (:493: NTT, not INTT)
    assert np.array_equal(enc.add_pt_to_ct(1, pt, False, c0, True), oQ.binop("Add", c0, oQ.INTT(pt)))
    assert np.array_equal(enc.add_pt_to_ct(0, pt, True, c0, True), oQ.binop("Add", c0[:1], pt[:1]))


def test_decrypt_reduces_where_the_reference_does():
    """degree 8 passes i = 7 (the Reduce inside the loop); the result is canonical at every degree"""
    oQ, _ = K.rings(5, 2, 0)
    rng = np.random.default_rng(4)
    sk = K.uniform(rng, oQ.moduli, 32)
    for degree in (1, 2, 7, 8):
        ct = [K.uniform(rng, oQ.moduli, 32) for _ in range(degree + 1)]
        pt, level = ER.decrypt(oQ, sk, ct, 1, 0, 1)
        assert level == 0 and pt.shape == (1, 32) and int(pt.max()) < oQ.moduli[0]
        # Horner over Python integers: every MulCoeffsMontgomery carries a factor 2^-64
        q = oQ.moduli[0]
        rinv = pow(1 << 64, -1, q)
        acc = [int(x) for x in ct[degree][0]]
        for i in range(degree, 0, -1):
            acc = [(a * int(b) * rinv + int(c)) % q for a, b, c in zip(acc, sk[0], ct[i - 1][0])]
        assert [int(x) for x in pt[0]] == acc


def test_decrypt_of_degree_7_in_the_coefficient_domain_is_where_the_reference_is_not_exact():
    """decryptor.go:86-92 hands INTT the unreduced sum of NTTLazy words when degree & 7 == 7.  With the Reduce made first the result
    is the Horner value over the integers; the device returns that (include/hering_encryptor.h)"""
    oQ, _ = K.rings(6, 3, 0)
    rng = np.random.default_rng(71)
    sk = K.uniform(rng, oQ.moduli, 64)
    ct = [K.uniform(rng, oQ.moduli, 64) for _ in range(8)]
    exact, _ = ER.decrypt(oQ, sk, ct, 0, 0, 0, reduce_always=True)
    ntt_ct = [oQ.NTT(c[:1]) for c in ct]
    in_ntt, _ = ER.decrypt(oQ, sk, ntt_ct, 0, 0, 1)
    assert np.array_equal(exact, oQ.INTT(in_ntt))
