"""The ring-packing evaluator on the host (no GPU): the three identities the device kernels rest on, checked on the oracle; the
restatement tests/ringpack_ref.py decrypting within the reference's own bounds (core/rlwe/ring_packing_test.go); the new header's
symbols, trace ids, aliasing rows, Go and C++ mirrors.

Identities (include/hering_ringpack.h), standard ring of degree N, limb by limb, Montgomery form included:
 1. XPow2NTT[i][j] = (bit i of j ? q - w : w), w = RootsForward[(N >> (i+1)) + (j >> (i+1))]; XInvPow2NTT the same on RootsBackward;
 2. Split's maps: even[j] = 2^-1 (t[2j] + t[2j+1]), odd[j] = 2^-1 w^-1 (t[2j] - t[2j+1]), w^-1 = RootsBackward[N/2 + j];
 3. Merge's map: out[2j] = e[j] + w o[j], out[2j+1] = e[j] - w o[j], w = RootsForward[N/2 + j]."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from lattigo_amd import _lib
from oracle import oracle as O
from tests import ringpack_aliasing as RP
from tests import ringpack_ref as REF
from tests.helpers import rng_for, uniform_poly

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hering_ringpack.h")
NEW = ("he_ring_xpow2_ntt", "he_ring_split_ntt", "he_ring_merge_ntt", "he_ringpack_split", "he_ringpack_merge",
       "he_ringpack_expand_step", "he_ringpack_pack_pre", "he_ringpack_pack_post")


def _moduli():
    q, _ = O.GenModuli(13, [60, 45], [])  # = 1 mod 2^13: NTT-friendly up to logN 12; one above 2^58, one below 2^47
    q = list(q)
    assert q[0] > (1 << 58) and q[1] < (1 << 47)
    return q


def xpow2_from_roots(r: O.Ring, i, div):
    """identity 1"""
    N, j = r.N, np.arange(r.N)
    out = []
    for l, q in enumerate(r.moduli):
        w = (r.roots_backward(l) if div else r.roots_forward(l))[(N >> (i + 1)) + (j >> (i + 1))]
        out.append(np.where((j >> i) & 1 == 1, np.uint64(q) - w, w))
    return np.stack(out).astype(np.uint64)


def _plain(w, q):
    """Montgomery form -> plain residues, as Python integers"""
    return (w.astype(object) * pow(1 << 64, -1, q)) % q


def split_butterfly(r: O.Ring, t):
    """identity 2 on [limbs][N] -> (even, odd) [limbs][N/2]"""
    n = r.N // 2
    ev, od = [], []
    for l, q in enumerate(r.moduli[: t.shape[0]]):
        a, b = t[l, 0::2].astype(object), t[l, 1::2].astype(object)
        winv = _plain(r.roots_backward(l)[n: 2 * n], q)
        h = pow(2, -1, q)
        ev.append((h * (a + b)) % q)
        od.append((h * winv * (a - b)) % q)
    return np.array(ev, dtype=np.uint64), np.array(od, dtype=np.uint64)


def merge_butterfly(r: O.Ring, e, o):
    """identity 3 on [limbs][N/2] x 2 -> [limbs][N]"""
    n = r.N // 2
    out = np.zeros((e.shape[0], r.N), dtype=np.uint64)
    for l, q in enumerate(r.moduli[: e.shape[0]]):
        w = _plain(r.roots_forward(l)[n: 2 * n], q)
        t = (w * o[l].astype(object)) % q
        out[l, 0::2] = np.array((e[l].astype(object) + t) % q, dtype=np.uint64)
        out[l, 1::2] = np.array((e[l].astype(object) - t) % q, dtype=np.uint64)
    return out


@pytest.mark.parametrize("logN", range(5, 13))
def test_identities_on_the_oracle(logN):
    q = _moduli()
    N = 1 << logN
    r, small = O.Ring(N, q), O.Ring(N // 2, q)
    rng = rng_for(8000 + logN)
    for div in (False, True):
        tabs = REF.GenXPow2NTT(r, logN, div)
        for i in range(logN):
            assert np.array_equal(tabs[i], xpow2_from_roots(r, i, div)), (logN, i, div)
    xinv0, x0 = REF.GenXPow2NTT(r, 1, True)[0], REF.GenXPow2NTT(r, 1, False)[0]
    top = np.array([[qi - 1] * N for qi in q], dtype=np.uint64)
    for t in (uniform_poly(rng, q, N), top):
        ev, od = split_butterfly(r, t)
        assert np.array_equal(ev, REF.switch_down_ntt(t, r, N // 2)), ("split even", logN)
        assert np.array_equal(od, REF.switch_down_ntt(r.binop("MulCoeffsMontgomery", t, xinv0), r, N // 2)), ("split odd", logN)
        # in coefficients: INTT_N(t)[0::2] and [1::2]
        c = r.INTT(t)
        assert np.array_equal(small.INTT(ev), c[:, 0::2]) and np.array_equal(small.INTT(od), c[:, 1::2])
    tops = top[:, : N // 2]
    for e, o in ((uniform_poly(rng, q, N // 2), uniform_poly(rng, q, N // 2)), (tops, tops)):
        want = r.binop("MulCoeffsMontgomeryThenAdd", REF.switch_up_ntt(o, 2), x0, REF.switch_up_ntt(e, 2))
        assert np.array_equal(merge_butterfly(r, e, o), want), ("merge", logN)


# ---- the restatement decrypts within the reference's bounds (ring_packing_test.go: logN 10 -> 8, one 60-bit Q, one 60-bit P) ----
LOGN_LARGE, LOGN_SMALL = 10, 8


@pytest.fixture(scope="module")
def setup():
    q, p = O.GenModuli(LOGN_LARGE + 1, [60], [60])
    rng = rng_for(8100)
    rings, sk, rsk, ext, rep = REF.gen_test_keys(rng, LOGN_LARGE, LOGN_SMALL, list(q), list(p), extract_at=(LOGN_SMALL,),
                                                 repack_at=(LOGN_SMALL, LOGN_LARGE))
    ev = REF.RingPackingEvaluator(rings, rsk, ext, rep)
    return dict(rng=rng, rings=rings, sk=sk, ev=ev, N=1 << LOGN_LARGE)


def _fresh(S):
    N = S["N"]
    pt = REF.gen_plaintext(N)
    return pt, REF.encrypt(S["rng"], S["rings"][LOGN_LARGE][0], S["sk"][LOGN_LARGE].Q, pt)


def test_ref_split_and_merge_decrypt(setup):
    S = setup
    pt, ct = _fresh(S)
    even, odd = S["ev"].Split(ct)
    rH, skH = S["rings"][LOGN_LARGE - 1][0], S["sk"][LOGN_LARGE - 1].Q
    for half, ref in ((even, pt[0::2]), (odd, pt[1::2])):
        err = REF.decrypt_centered(rH, half, skH) - ref
        assert REF.log2_std(err) <= LOGN_LARGE - 1 + 1          # ring_packing_test.go:126-127
    n = S["N"] // 2
    pe, po = REF.gen_plaintext(n), REF.gen_plaintext(n)
    cte, cto = REF.encrypt(S["rng"], rH, skH, pe), REF.encrypt(S["rng"], rH, skH, po)
    ctN = S["ev"].Merge(cte, cto)
    got = REF.decrypt_centered(S["rings"][LOGN_LARGE][0], ctN, S["sk"][LOGN_LARGE].Q)
    got[0::2] -= pe
    got[1::2] -= po
    assert REF.log2_std(got) <= LOGN_LARGE + 1                  # :179


@pytest.mark.parametrize("naive", [False, True])
def test_ref_extract_decrypts(setup, naive):
    S = setup
    pt, ct = _fresh(S)
    gap = 17
    log_gap = gap.bit_length()                                  # bits.Len64(17) = 5, :197
    idx = [i * gap for i in range(S["N"] // gap)]
    cts = S["ev"].extract(ct, idx, naive)
    assert sorted(cts) == idx
    rS, skS = S["rings"][LOGN_SMALL][0], S["sk"][LOGN_SMALL].Q
    for i in idx:
        assert cts[i].shape[2] == 1 << LOGN_SMALL
        d = REF.decrypt_centered(rS, cts[i], skS)
        d[0] -= int(pt[i])
        if naive:
            assert np.log2(max(abs(int(d[0])), 1)) <= LOGN_LARGE           # :316-318
        else:
            assert REF.log2_std(d) <= LOGN_LARGE + log_gap + 1             # :244


def test_ref_repack_decrypts(setup):
    S = setup
    N = S["N"]
    rQ, skQ = S["rings"][LOGN_LARGE][0], S["sk"][LOGN_LARGE].Q
    pt = REF.gen_plaintext(N)
    gap = 3
    cts = {}
    for i in range(0, N, gap):  # ciphertext i holds pt * X^-i: its constant coefficient is pt[i] (:341-352)
        rot = np.concatenate([pt[i:], -pt[:i]])
        cts[i] = REF.encrypt(S["rng"], rQ, skQ, rot)
    ct = S["ev"].Repack(cts)
    got = REF.decrypt_centered(rQ, ct, skQ)
    got[0::gap] -= pt[0::gap]
    assert REF.log2_std(got) <= LOGN_LARGE + 5                  # :382


@pytest.mark.parametrize("extract_naive,repack_naive", [(False, True), (True, False)])
def test_ref_extract_permute_repack(setup, extract_naive, repack_naive):
    S = setup
    N = S["N"]
    pt, ct = _fresh(S)
    idx = sorted(int(x) for x in rng_for(8200).permutation(N)[: N // 2])
    cts = S["ev"].extract(ct, idx, extract_naive)
    assert all(c.shape[2] == 1 << LOGN_SMALL for c in cts.values())
    permute = lambda x: (x + N // 2) & (N - 1)
    out = S["ev"].repack({permute(i): c for i, c in cts.items()}, repack_naive)
    got = REF.decrypt_centered(S["rings"][LOGN_LARGE][0], out, S["sk"][LOGN_LARGE].Q)
    for k0 in idx:
        got[permute(k0)] -= int(pt[k0])
    assert REF.log2_std(got) <= LOGN_LARGE + 5                  # :486


def test_get_minimum_gap_and_galois_elements():
    from lattigo_amd import rlwe as R
    for lst in ([0, 17, 34], [0, 4, 12], [3, 11, 12], [0, 6, 12, 48]):
        assert R.getMinimumGap(lst) == REF.getMinimumGap(lst)
    with pytest.raises(ValueError):
        R.getMinimumGap([0, 0])
    with pytest.raises(ValueError):
        R.getMinimumGap([1, 0])
    assert R.GaloisElementsForExpand(2048, 10) == REF.GaloisElementsForExpand(1024, 10)
    for lg in (0, 3, 10):
        assert R.GaloisElementsForPack(2048, 10, lg) == REF.GaloisElementsForPack(1024, lg)


# ---- the layers -------------------------------------------------------------------------------------------------------------------
def test_header_symbols_declared_and_exported():
    syms = _lib.declared_symbols()
    for s in NEW:
        assert s in syms, s
    assert os.path.exists(_lib.lib_path()), "libhering.so is not built"
    L = _lib.load()
    missing = [s for s in NEW if not hasattr(L, s)]
    assert not missing, missing
    for s in NEW:
        assert getattr(L, s).argtypes is not None, s


def test_trace_ids_follow_the_existing_ones():
    ids = [_lib._TRACE_FNS[s][0] for s in NEW]
    assert ids == list(range(55, 55 + 8)), ids
    old = {k: v[0] for k, v in _lib._TRACE_FNS.items() if k not in NEW}
    assert max(old.values()) == 54 and old["he_apply_evaluation_key"] == 54 and old["he_poly_alloc"] == 0
    replay = open(os.path.join(ROOT, "lattigo_amd", "csrc", "replay.cpp")).read()
    for s in NEW:
        assert re.search(r"\b%s\(" % s, replay), s


def test_aliasing_rows_are_the_header_entry_points():
    from tests.test_aliasing_table import poly_entries
    entries = poly_entries(open(HEADER).read())
    assert sorted(entries) == sorted(RP.ROWS), (sorted(entries), sorted(RP.ROWS))
    for name, params in entries.items():
        assert list(RP.ROWS[name].params) == params, (name, params)
    # the rules the header states
    for name, row in RP.ROWS.items():
        outs = [p for p in row.params if row.written(p)]
        for a in outs:
            for b in outs:
                if a != b:
                    assert row.verdict(a, b) == "reject", (name, a, b)
    es = RP.ROWS["he_ringpack_expand_step"]
    assert es.verdict("out0", "in0") == "accept" and es.verdict("out1", "in1") == "accept"
    assert es.verdict("out0", "tmp0") == "reject" and es.verdict("out0", "in1") == "reject"
    assert RP.ROWS["he_ringpack_split"].verdict("even0", "in0") == "reject"
    assert RP.ROWS["he_ringpack_merge"].verdict("even0", "odd0") == "accept"


def test_check_go_abi_lists_split_and_merge():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_go_abi.py")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert re.search(r"RingPackingEvaluator: .*\bSplit\b.*\bMerge\b", out.stdout), out.stdout
    go = open(os.path.join(ROOT, "go", "hering", "ringpack.go")).read()
    for s in NEW:
        assert re.search(r"C\.%s\(" % s, go), s


def test_cpp_mirror_compiles_with_the_new_methods():
    src = os.path.join(ROOT, "tests", "cpp", "ringpack_mirror.cpp")
    text = open(src).read()
    for m in ("SplitNew", "MergeNew", ".Split(", ".Merge(", "XPow2NTT", "SplitNTT", "MergeNTT", "ExpandStep", "PackPre", "PackPost"):
        assert m in text, m
    hpp = open(os.path.join(ROOT, "include", "hering.hpp")).read()
    for s in NEW:
        assert re.search(r"\b%s\(" % s, hpp), s
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
