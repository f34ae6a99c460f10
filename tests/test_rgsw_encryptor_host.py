"""The restatement of rgsw.Encryptor and blindrot.GenEvaluationKeyNew (tests/rgsw_encryptor_ref.py) held against what an RGSW
ciphertext is, the cases of the GPU tests (tests/rgsw_encryptor_cases.py) held against the exp / log condition they rest on, and
the header's symbols.  No GPU."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as graft
from lattigo_amd import _lib
from tests import keygen_cases as K
from tests import keygen_ref as KR
from tests import rgsw_encryptor_aliasing as A
from tests import rgsw_encryptor_cases as GC
from tests import rgsw_encryptor_ref as GR
from tests import sampler_ref as R
from tests.encryptor_cases import centered

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hering_rgsw_encryptor.h")
ENTRIES = ["he_blindrot_gen_evaluation_key", "he_rgsw_encrypt", "he_rgsw_encrypt_table", "he_rgsw_encrypt_zero"]


@pytest.fixture(scope="module")
def lib():
    graft.build()
    return _lib.load()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ---- what an RGSW ciphertext is ---------------------------------------------------------------------------------------------------------
def assert_rgsw_rows(c: K.Case, ct, gaussians, pt, sk=None):
    """The big-integer statement, limb by limb (a polynomial that is the same small centred value on every Q and P limb is that
    small polynomial modulo QP).  With s the secret and g_ij = P 2^(j pw2) on the Q limbs of the row's digit, 0 elsewhere:
        Value[0][i][j]: c0 + c1 s - pt g_ij        Value[1][i][j]: c0 + (c1 - pt g_ij) s
    are polynomials of centred infinity norm at most 19 -- Xe = {3.2, 19.2} and the sampler's uint64(v + 0.5) with v <= 19.2 --
    and the Gaussians the restatement recorded.  pt: Montgomery words (the term is then pt g_ij word by word) or None."""
    oQ, oP = K.rings(c)
    skQ, skP = sk or K.secret(c)
    rows = KR.gadget_rows(c.Q, c.levelQ, c.levelP, c.pw2)
    assert len(rows) == c.rows == ct[0]["q"].shape[0] == ct[1]["q"].shape[0]
    P = math.prod(c.P[:c.levelP + 1])
    alpha = max(c.levelP + 1, 1)
    for u in range(2):
        assert len(gaussians[u]) == len(rows)
        for r, (i, j) in enumerate(rows):
            c0, c1 = ct[u]["q"][r, 0].copy(), ct[u]["q"][r, 1].copy()
            term = np.zeros_like(c0)
            for k in range(alpha):
                index = i * alpha + k
                if index > c.levelQ or pt is None:
                    break
                q = c.Q[index]
                f = P * (1 << (j * c.pw2)) % q
                term[index] = np.array([int(w) * f % q for w in pt[index]], dtype=np.uint64)
            if u == 0:
                x = oQ.binop("Sub", oQ.binop("MulCoeffsMontgomeryThenAdd", c1, skQ[:c.levelQ + 1], c0), term)
            else:
                x = oQ.binop("MulCoeffsMontgomeryThenAdd", oQ.binop("Sub", c1, term), skQ[:c.levelQ + 1], c0)
            e = oQ.unop("IMForm", oQ.INTT(x))
            small = centered(gaussians[u][r][0], c.Q[0])
            assert max(abs(v) for v in small) <= 19 and any(small)
            for limb in range(c.levelQ + 1):
                assert centered(e[limb], c.Q[limb]) == small, (u, r, "Q", limb)
            if c.levelP >= 0:
                y = oP.unop("IMForm", oP.INTT(oP.binop("MulCoeffsMontgomeryThenAdd", ct[u]["p"][r, 1], skP[:c.levelP + 1], ct[u]["p"][r, 0])))
                for limb in range(c.levelP + 1):
                    assert centered(y[limb], c.P[limb]) == small, (u, r, "P", limb)


@pytest.mark.parametrize("c", GC.CASES, ids=lambda c: c.id)
def test_rows_of_an_rgsw_ciphertext(c):
    ct, gaussians, pos = GC.want_encrypt(c)
    assert_rgsw_rows(c, ct, gaussians, GC.plaintext(c))
    assert pos > 0
    assert not np.array_equal(ct[0]["q"][:, 1], ct[1]["q"][:, 1])


def test_rows_of_an_encryption_of_zero():
    c = GC.ORDER_CASE
    ct, gaussians, pos = GC.want_zero(c)
    assert_rgsw_rows(c, ct, gaussians, None)
    full, _, pos2 = GC.want_encrypt(c)
    # the same stream: the plaintext moves component 0 of Value[0] and component 1 of Value[1] on the digit limbs and nothing else
    assert pos == pos2 and np.array_equal(ct[0]["q"][:, 1], full[0]["q"][:, 1]) and np.array_equal(ct[1]["q"][:, 0], full[1]["q"][:, 0])
    assert np.array_equal(ct[0]["p"], full[0]["p"]) and np.array_equal(ct[1]["p"], full[1]["p"])
    assert not np.array_equal(ct[0]["q"][:, 0], full[0]["q"][:, 0]) and not np.array_equal(ct[1]["q"][:, 1], full[1]["q"][:, 1])


@pytest.mark.parametrize("form", [(False, False), (True, False), (False, True)], ids=["coefficients", "ntt", "coefficients-montgomery"])
def test_plaintext_forms(form):
    """the three branches of :47-60 bring the plaintext to NTT and Montgomery form before the gadget term"""
    c = GC.FORMS_CASE
    oQ, _ = K.rings(c)
    ct, gaussians, _ = GC.want_encrypt(c, form)
    pt = GC.plaintext(c)
    if not form[0]:
        pt = oQ.NTT(pt)
    if not form[1]:
        pt = oQ.unop("MForm", pt)
    assert_rgsw_rows(c, ct, gaussians, pt)


def test_table_is_its_ciphertexts_in_order():
    c, sel, m = GC.TABLE_CASE, GC.TABLE_SEL, GC.TABLE_M
    cts, gaussians, pos = GC.want_table(c, tuple(sel), m)
    pts = GC.table_plaintexts(c, m)
    for ct, g, s in zip(cts, gaussians, sel):
        assert_rgsw_rows(c, ct, g, None if s < 0 else pts[s])
    # one source, ciphertext after ciphertext: the first is the ciphertext an encryptor makes alone from the same stream
    enc, src = GC.encryptor(c, c.seed + 2000)
    assert GC.same_ct(enc.encrypt(pts[sel[0]], True, True, c.levelQ, c.levelP, c.pw2), cts[0]) and 0 < src.pos < pos


def test_blind_rotation_keys_encrypt_the_monomials_of_the_lwe_secret():
    c = GC.E2E_CASE
    oQ, _ = K.rings(c)
    brk, gks, (g_rgsw, g_gal), (pos, pos_kg) = GC.want_blindrot(False)
    s = GR.centered_lwe_secret(GC.lwe_ring(), GC.lwe_secret())
    assert len(brk) == GC.N_LWE == len(s) and set(s) <= {-1, 0, 1} and len(set(s)) > 1
    for ct, g, si in zip(brk, g_rgsw, s):
        assert_rgsw_rows(c, ct, g, oQ.unop("MForm", oQ.NTT(GR.monomial(oQ, si))))
    assert list(gks) == GR.galois_elements(c.N) and len(gks) == GR.WINDOW_SIZE + 1 and pos > 0 and pos_kg > 0
    # on one source the RGSW ciphertexts draw first and the Galois keys after them
    brk1, gks1, _, (pos1, _) = GC.want_blindrot(True)
    assert all(GC.same_ct(a, b) for a, b in zip(brk, brk1)) and pos1 > pos
    assert not K.same_key(gks[5], gks1[5])


def test_monomials_wrap_as_new_monomial_xi():
    oQ, _ = K.rings(K.C_B16_NOP)
    N, q = oQ.N, [int(x) for x in oQ.moduli]
    for i, (at, w) in {0: (0, 1), 1: (1, 1), -1: (N - 1, -1), N - 1: (N - 1, 1), N: (0, -1), -N: (0, -1), 2 * N + 3: (3, 1), N + 2: (2, -1)}.items():
        p = GR.monomial(oQ, i)
        for k in range(len(q)):
            assert int(p[k, at]) == (1 if w == 1 else q[k] - 1) and np.count_nonzero(p[k]) == 1, (i, k)


def test_lwe_secret_is_centred_at_half_the_modulus():
    """PolyToBigintCentered: a word >= q0 >> 1 is taken minus q0"""
    rl = GC.lwe_ring()
    q0 = GC.Q_LWE
    vals = [0, 1, (q0 >> 1) - 1, q0 >> 1, (q0 >> 1) + 1, q0 - 1] + [0] * (GC.N_LWE - 6)
    w = rl.unop("MForm", rl.NTT(np.array([vals], dtype=np.uint64)))
    assert GR.centered_lwe_secret(rl, w)[:6] == [0, 1, (q0 >> 1) - 1, (q0 >> 1) - q0, (q0 >> 1) + 1 - q0, -1]


# ---- the stream check the GPU tests rest on ----------------------------------------------------------------------------------------------
def _same(a, b):
    return GC.same_ct(a[0], b[0]) and a[2] == b[2] and all(np.array_equal(x, y) for u in range(2) for x, y in zip(a[1][u], b[1][u]))


def _shifted(ulps):
    return R.shifted(math.exp, ulps), R.shifted(R._log, ulps)


@pytest.mark.parametrize("c", GC.CASES, ids=lambda c: c.id)
def test_no_ciphertext_depends_on_exp_or_log(c):
    base = GC.want_encrypt(c)
    for ulps in (4, -4):
        assert _same(base, GC.run_encrypt(c, (True, True), *_shifted(ulps))), ulps


def test_no_other_case_depends_on_exp_or_log():
    for ulps in (4, -4):
        sh = _shifted(ulps)
        assert _same(GC.want_zero(GC.ORDER_CASE), GC.run_zero(GC.ORDER_CASE, *sh)), ulps
        for form in ((False, False), (True, False)):
            assert _same(GC.want_encrypt(GC.FORMS_CASE, form), GC.run_encrypt(GC.FORMS_CASE, form, *sh)), (form, ulps)
        for c, sel, m in ((GC.TABLE_CASE, GC.TABLE_SEL, GC.TABLE_M), (K.C_REJECT, GC.REJECT_TABLE_SEL, 1)):
            cts, _, pos = GC.want_table(c, tuple(sel), m)
            cts2, _, pos2 = GC.run_table(c, sel, m, *sh)
            assert pos == pos2 and all(GC.same_ct(a, b) for a, b in zip(cts, cts2)), (c.id, ulps)


def test_the_blind_rotation_keys_do_not_depend_on_exp_or_log():
    for one in (False, True):
        brk, gks, _, pos = GC.want_blindrot(one)
        for ulps in (4, -4):
            brk2, gks2, _, pos2 = GC.run_blindrot(one, *_shifted(ulps))
            assert pos == pos2 and all(GC.same_ct(a, b) for a, b in zip(brk, brk2)), (one, ulps)
            assert all(K.same_key(gks[g], gks2[g]) for g in gks), (one, ulps)


def test_the_rejecting_modulus_rejects_inside_the_table():
    c = K.C_REJECT
    _, _, pos = GC.want_table(c, tuple(GC.REJECT_TABLE_SEL), 1)
    per_row = 8 * ((2 * c.N + 127) // 128 * 128 + (c.N + 127) // 128 * 128) + (8 * c.N + 1023) // 1024 * 1024
    assert pos > len(GC.REJECT_TABLE_SEL) * 2 * c.rows * per_row


# ---- the header ---------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_exported_and_left_out_of_recordings(lib):
    mine = sorted(set(re.findall(r"\b(he_[a-z0-9_]+)\s*\(", _header())))
    assert mine == ENTRIES and all(s in _lib.declared_symbols() and hasattr(lib, s) for s in mine), mine
    tables = (_lib._TRACE_FNS, _lib._TRACE_FNS_RGSW, _lib._TRACE_FNS_BLINDROT, _lib._TRACE_FNS_BRIDGE, _lib._TRACE_FNS_BFV)
    for s in mine:
        assert not any(s in t for t in tables), s  # no replay numbers
        assert s in _lib._TRACE_IGNORE, s
    names = [lib.he_prof_kernel_name(i).decode() for i in range(64)]
    assert names.index("rgsw_table_finish") == names.index("gadget_add") + 1


def test_go_shim_defines_the_entries():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_go_abi.py")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "hering_rgsw_encryptor.h" in open(os.path.join(ROOT, "tools", "check_go_abi.py")).read()
    src = "".join(open(os.path.join(ROOT, "go", "hering", f)).read() for f in sorted(os.listdir(os.path.join(ROOT, "go", "hering"))) if f.endswith(".go"))
    for name in ENTRIES:
        assert "C." + name + "(" in src, name
    for method in ("func (enc *RGSWEncryptor) Encrypt(", "func (enc *RGSWEncryptor) EncryptZero(", "func (enc *RGSWEncryptor) EncryptTable(",
                   "func GenBlindRotationEvaluationKeyNew("):
        assert method in src, method


def test_aliasing_table_covers_the_header():
    """every entry of the header has a row whose handle operands are the header's, in order; every output is distinct from every
    other output: no pair is allowed"""
    entries = {}
    for m in re.finditer(r"\bint\s+(he_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", _header(), flags=re.S):
        ops = [p.split()[-1].lstrip("*") for p in m.group(2).split(",") if "he_handle" in p and re.match(r"\*?(pts?|skLWE|rgsw[01]|gks)$", p.split()[-1])]
        entries[m.group(1)] = ops
    assert sorted(entries) == sorted(A.ROWS) == ENTRIES
    for name, ops in entries.items():
        row = A.ROWS[name]
        assert list(row.params) == ops, (name, ops)
        assert not row.allowed
        outs = [p for p in row.params if row.written(p)]
        for a in outs:
            for b in row.params:
                if a != b:
                    assert row.verdict(a, b) == "reject", (name, a, b)
    pairs = {(n, a, b) for n, a, b in A.PAIRS}
    for name, row in A.ROWS.items():
        outs = [p for p in row.params if row.written(p)]
        for i, a in enumerate(outs):
            for b in outs[i + 1:]:
                assert (name, a, b) in pairs, (name, a, b)
            if a in row.arrays:
                assert (name, a, a) in pairs, (name, a)
