"""The restatement of rlwe.KeyGenerator (tests/keygen_ref.py) held against what an evaluation key is, the sparse sampler against what
it promises, the cases of the GPU tests (tests/keygen_cases.py) held against the exp / log condition they rest on, and the header's
symbols.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

import __graft_entry__ as graft
from lattigo_amd import _lib
from tests import keygen_aliasing as A
from tests import keygen_cases as K
from tests import keygen_ref as KR
from tests import sampler_ref as R
from tests.encryptor_cases import centered

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hering_keygen.h")
HANDLES = {"he_keygen_create", "he_keygen_destroy"}


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ---- what an evaluation key is --------------------------------------------------------------------------------------------------------
def assert_rows_decrypt_to_their_gaussians(c: K.Case, key, gaussians, operands):
    """row (i, j): IMForm(INTT(c0 + c1 skOut)) minus the gadget term, centred, is one small polynomial on every Q and P limb, within
    the bound, and the Gaussian the restatement recorded for the row"""
    oQ, oP = K.rings(c)
    skIn, (skOutQ, skOutP) = operands
    rows = KR.gadget_rows(c.Q, c.levelQ, c.levelP, c.pw2)
    assert len(rows) == c.rows == key["q"].shape[0] == len(gaussians)
    P = math.prod(c.P[:c.levelP + 1])
    alpha = max(c.levelP + 1, 1)
    for r, (i, j) in enumerate(rows):
        x = oQ.binop("MulCoeffsMontgomeryThenAdd", key["q"][r, 1], skOutQ[:c.levelQ + 1], key["q"][r, 0])
        for k in range(alpha):  # the term of the row's digit: skIn (Montgomery form) times P 2^(j pw2)
            index = i * alpha + k
            if index > c.levelQ:
                break
            q = c.Q[index]
            f = P * (1 << (j * c.pw2)) % q
            x[index] = np.array([(int(w) - int(s) * f) % q for w, s in zip(x[index], skIn[index])], dtype=np.uint64)
        e = oQ.unop("IMForm", oQ.INTT(x))
        small = centered(gaussians[r][0], c.Q[0])
        assert max(abs(v) for v in small) <= 19 and any(small)  # the floor of the bound 19.2
        for limb in range(c.levelQ + 1):
            assert centered(e[limb], c.Q[limb]) == small, (r, "Q", limb)
        if c.levelP >= 0:
            y = oP.unop("IMForm", oP.INTT(oP.binop("MulCoeffsMontgomeryThenAdd", key["p"][r, 1], skOutP[:c.levelP + 1], key["p"][r, 0])))
            for limb in range(c.levelP + 1):
                assert centered(y[limb], c.P[limb]) == small, (r, "P", limb)


@pytest.mark.parametrize("c", K.RLK_CASES, ids=lambda c: c.id)
def test_rows_of_a_relinearization_key(c):
    key, gaussians, pos, operands = K.want_rlk(c)
    assert_rows_decrypt_to_their_gaussians(c, key, gaussians, operands)
    assert pos > 0


@pytest.mark.parametrize("c", K.GALOIS_CASES, ids=lambda c: c.id)
def test_rows_of_the_galois_keys(c):
    for g in K.galois_elements(c):
        key, gaussians, _, operands = K.want_galois(c, g)
        assert_rows_decrypt_to_their_gaussians(c, key, gaussians, operands)


def test_rows_of_a_set_of_galois_keys_and_its_stream():
    c = K.GALOIS_SET_CASE
    keys, gaussians, pos, operands = K.want_galois_set(c)
    for key, gs, ops in zip(keys, gaussians, operands):
        assert_rows_decrypt_to_their_gaussians(c, key, gs, ops)
    assert not K.same_key(keys[0], keys[1])
    # one source, key after key: the first key of the set is the key a generator makes alone from the same stream
    kg, _ = K.generator(c, c.seed + 300)
    assert K.same_key(kg.gen_galois_key(K.galois_elements(c)[0], K.secret(c), c.levelQ, c.levelP, c.pw2), keys[0])


@pytest.mark.parametrize("up", [True, False])
def test_rows_of_a_key_between_two_ring_degrees(up):
    c = K.C_SWITCH
    key, gaussians, _, operands = K.want_switch(c, up)
    assert_rows_decrypt_to_their_gaussians(c, key, gaussians, operands)
    skIn, (skOutQ, skOutP) = operands
    small = np.repeat(K.small_secret(c), c.N >> K.SMALL_LOGN, axis=1)
    assert np.array_equal(skIn if up else skOutQ, small) and np.array_equal(skOutQ if up else skIn, K.secret(c)[0])
    assert up is False or np.array_equal(skOutP, K.secret(c)[1])  # the rebuilt P part is the key's own
    for ulps in (4, -4):
        assert _same(K.want_switch(c, up), K.run_switch(c, up, R.shifted(math.exp, ulps), R.shifted(R._log, ulps))), ulps


def test_the_rejecting_modulus_rejects_and_moves_the_rows():
    """about half of the words of limb 0 are rejected, so a row does not start where a parse without rejections would put it"""
    c = K.C_REJECT
    _, _, pos, _ = K.want_rlk(c)
    per_row = 8 * ((2 * c.N + 127) // 128 * 128 + (c.N + 127) // 128 * 128) + (8 * c.N + 1023) // 1024 * 1024
    assert pos > c.rows * per_row


# ---- the sparse sampler ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [1, 8, 9, 31, 32, 37])
@pytest.mark.parametrize("montgomery", [False, True])
def test_sparse_sampler(hw, montgomery):
    N, moduli = 32, K.C_3P2.Q[:2]
    src, tr = R.seeded_source(900 + hw), KR.SparseTrace()
    pol = KR.sample_sparse(src, N, moduli, hw, montgomery, tr)
    n = min(hw, N)
    for limb, q in zip(pol, moduli):
        one, minus = (R.mform(1, q), R.mform(q - 1, q)) if montgomery else (1, q - 1)
        assert sum(1 for w in limb if w != 0) == n and set(limb) <= {0, one, minus}
    assert [w != 0 for w in pol[0]] == [w != 0 for w in pol[1]]
    assert tr.draws - tr.rejected == n
    assert src.pos == (n + 7) // 8 + 4 * tr.draws  # no buffer rounding: the reference reads these straight from the source
    if hw == 37:
        assert pol == KR.sample_sparse(R.seeded_source(900 + hw), N, moduli, N, montgomery)  # hw > N clamps to N


def test_sparse_secret_key_has_its_weight():
    c = K.C_3P2
    (skQ, skP), pos = K.want_sk(c, K.sk_hw(c))
    oQ, oP = K.rings(c)
    s = centered(oQ.unop("IMForm", oQ.INTT(skQ))[0], c.Q[0])
    assert sum(1 for v in s if v) == K.sk_hw(c) and set(s) <= {-1, 0, 1}
    assert centered(oP.unop("IMForm", oP.INTT(skP))[1], c.P[1]) == s and pos > 0


# ---- the stream check the GPU tests rest on ----------------------------------------------------------------------------------------------
def _same(a, b):
    return K.same_key(a[0], b[0]) and a[2] == b[2] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("c", K.RLK_CASES, ids=lambda c: c.id)
def test_no_relinearization_key_depends_on_exp_or_log(c):
    base = K.want_rlk(c)
    for ulps in (4, -4):
        assert _same(base, K.run_rlk(c, R.shifted(math.exp, ulps), R.shifted(R._log, ulps))), ulps


@pytest.mark.parametrize("c", K.GALOIS_CASES, ids=lambda c: c.id)
def test_no_galois_key_depends_on_exp_or_log(c):
    for g in K.galois_elements(c):
        base = K.want_galois(c, g)
        for ulps in (4, -4):
            assert _same(base, K.run_galois(c, g, R.shifted(math.exp, ulps), R.shifted(R._log, ulps))), (g, ulps)


def test_the_set_of_galois_keys_does_not_depend_on_exp_or_log():
    c = K.GALOIS_SET_CASE
    keys, _, pos, _ = K.want_galois_set(c)
    for ulps in (4, -4):
        keys2, _, pos2, _ = K.run_galois_set(c, R.shifted(math.exp, ulps), R.shifted(R._log, ulps))
        assert pos == pos2 and all(K.same_key(a, b) for a, b in zip(keys, keys2)), ulps


# ---- the gadget term alone --------------------------------------------------------------------------------------------------------------
def test_gadget_term_of_two_keys_goes_to_component_u_of_key_u():
    c = K.C_B16
    oQ, oP = K.rings(c)
    rng = np.random.default_rng(5)
    pt = np.stack([rng.integers(0, q, c.N, dtype=np.uint64) for q in c.Q])
    keys = [np.zeros((c.rows, 2, c.levelQ + 1, c.N), dtype=np.uint64) for _ in range(2)]
    KR.add_poly_times_gadget_vector(oQ, oP, pt, keys, c.levelQ, c.levelP, c.pw2)
    assert not keys[0][:, 1].any() and not keys[1][:, 0].any() and np.array_equal(keys[0][:, 0], keys[1][:, 1])
    rows = KR.gadget_rows(c.Q, c.levelQ, c.levelP, c.pw2)
    for r, (i, j) in enumerate(rows):
        for limb, q in enumerate(c.Q):
            want = [int(w) * c.P[0] * (1 << (16 * j)) % q if limb == i else 0 for w in pt[limb]]
            assert [int(w) for w in keys[0][r, 0, limb]] == want, (r, limb)


# ---- the header ---------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_exported_and_left_out_of_recordings(lib):
    mine = sorted(set(re.findall(r"\b(he_[a-z0-9_]+)\s*\(", _header())))
    assert len(mine) >= 11 and all(s in _lib.declared_symbols() and hasattr(lib, s) for s in mine), mine
    tables = (_lib._TRACE_FNS, _lib._TRACE_FNS_RGSW, _lib._TRACE_FNS_BLINDROT, _lib._TRACE_FNS_BRIDGE, _lib._TRACE_FNS_BFV)
    for s in mine:
        assert not any(s in t for t in tables), s  # no replay numbers
        assert (s in _lib._TRACE_IGNORE) == (s in HANDLES), s  # a generation entry draws from the source: it fails a recording
    names = [lib.he_prof_kernel_name(i).decode() for i in range(64)]
    assert names.index("gadget_add") == names.index("evk_finish") + 1 == names.index("sampler_expand") + 2


def test_prototypes_live_in_the_new_header_only():
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h.endswith((".h", ".hpp")) and h != "hering_keygen.h":
            src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
            src = re.sub(r"//[^\n]*", "", src)
            assert not re.search(r"\bint\s+he_(keygen_[a-z0-9_]*|gadget_add_poly)\s*\(", src), h


def test_aliasing_table_covers_the_header():
    """every entry of the header with a polynomial or key operand has a row whose parameters are the header's, in order"""
    entries = {}
    for m in re.finditer(r"\bint\s+(he_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", _header(), flags=re.S):
        ops = [p.split()[-1].lstrip("*") for p in m.group(2).split(",")
               if "he_handle" in p and re.match(r"\*?(sk\w*|pol|pt|evk\d?|rlk|gk|gks)$", p.split()[-1])]
        if ops:
            entries[m.group(1)] = ops
    assert sorted(entries) == sorted(A.ROWS)
    for name, ops in entries.items():
        assert list(A.ROWS[name].params) == ops, (name, ops)
