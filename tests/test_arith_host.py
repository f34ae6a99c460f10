"""The arithmetic primitives without a device (tests/arith_ref.py holds the references and the operand sets; tests/test_gpu_arith.py
runs the same sets through he_debug_arith on the GPU):

* the conditions on the operand sets: no family empty after clipping to the op's domain, at most 2^17 tuples, 2^16 random ones, a
  tuple of each kind in the zero-round family, and -- at every integer-class modulus -- both values of each of the four carries of
  the column schedule (where interval arithmetic shows that a carry cannot be one at that modulus, it must be zero throughout:
  arith_ref.carries_reachable);
* the written argument of the two word-serial Montgomery forms, restated: no 64-bit accumulator overflows on the callers' domain
  (x < 4q at q < 2^61, x < 34q at q < 2^58), and the column form DOES overflow just past it (x < 63q at the largest prime below
  2^58): the 34q bound is load-bearing;
* every expected word against the truth in Python integers (residue class, stated range map), on every set;
* csrc/modarith.h itself as a host program (tests/cpp/modarith_host.cpp, plain g++) on the same sets against the same words.

Nothing here skips, filters or tolerates a tuple: every comparison is exact."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests import arith_ref as A
from tests.helpers import rng_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
MODS = {name: q for name, q, _, _ in A.moduli()}
U = np.uint64


def test_moduli_cover_the_class_edges_and_the_word_edge():
    m = MODS
    assert len(m) == 9
    assert m["top61"] < 1 << 61 and m["top61"] >= m["qi60_0"] > 1 << 60
    assert m["max58"] < 1 << 58 <= m["min58"] and m["max47"] < 1 << 47 <= m["min47"]
    assert m["min32"] >> 32 == 1 and m["max32"] >> 32 == 0 and m["max32"] >> 31 == 1 and m["q27"].bit_length() == 27
    assert m["min58"] - (1 << 58) < 1 << 18 and (1 << 58) - m["max58"] < 1 << 18
    # one ring per arithmetic class, limbs numbered in order
    assert sorted((c, l) for _, _, c, l in A.moduli()) == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2)]


@pytest.mark.parametrize("name", list(MODS))
def test_constants_against_the_oracle(name):
    q = MODS[name]
    k, o = A.consts(q), O.Ring(A.N, [q]).constants(0)
    assert (k.qinv, (k.brc0, k.brc1), k.ninv) == (o["qinv"], o["brc"], o["ninv"])
    assert k.rq_m * 2.0 ** k.rq_e == 1.0 / q  # ModConst::rq is the IEEE quotient (host_math.cpp)


def test_round_to_nearest_even_helper():
    rng = rng_for(7001)
    for bits in (10, 53, 54, 55, 64, 99, 100, 106):
        for _ in range(2000):
            v = A._ri(rng, 0, 1 << bits) - (1 << (bits - 1))
            assert A.rn_int(v) == int(float(v))  # CPython converts an integer to the nearest double, ties to even
    # ties: 2^53 + 1 -> 2^53 (even), 2^53 + 3 -> 2^53 + 4
    assert A.rn_int((1 << 53) + 1) == 1 << 53 and A.rn_int((1 << 53) + 3) == (1 << 53) + 4 and A.rn_int(-(1 << 53) - 1) == -(1 << 53)
    assert A.rne_shift(5, 1) == 2 and A.rne_shift(7, 1) == 4 and A.rne_shift(-5, 1) == -2 and A.rne_shift(-7, 1) == -4
    for num, den in ((1, 3), (1, (1 << 47) - 1), (2, 3), (1, 10), (1, 1 << 20), (7, (1 << 61) - 1)):
        m, e = A.rn_ratio(num, den)
        assert m * 2.0 ** e == num / den  # (CPython's true division of integers is correctly rounded)


SET_CASES = sorted({(kind, name) for op, name in A.cases() for kind in A.op_sets(op)})


@pytest.mark.parametrize("kind,name", SET_CASES)
def test_operand_sets(kind, name):
    """the generators assert the clipping; here: the families an op needs are there, none is empty, and the sizes"""
    q = MODS[name]
    fam = A.families(kind, q)
    want = {"lattice", "random"}
    if kind in ("mont", "w32", "keys", "fwd", "nc", "inv"):
        want |= {"zero", "top", "hunt"}
    if kind in ("hi128", "word", "word2", "halve"):
        want |= {"zero", "top"}
    if kind == "keys":
        want |= {"keys"}
    if kind in ("modmul", "modmul_wide", "f64x"):
        want |= {"half"}
    assert set(fam) == want
    assert all(len(cols[0]) > 0 for cols in fam.values())
    assert len(fam["random"][0]) == A.N_RANDOM
    assert sum(len(cols[0]) for cols in fam.values()) <= A.MAX_SET
    if kind in ("mont", "w32", "keys"):  # both kinds of zero round (the generator asserts each tuple's kind)
        x, y = fam["zero"]
        p = x * y
        assert ((p & U(0xFFFFFFFF)) == 0).any() and (p != 0).any() and (p == 0).any()
    if kind == "keys":
        x, y = fam["keys"]
        assert (y >= U(q)).all()


SCHEDULE_OPS = ("MRED_LAZY_W32", "MRED_LAZY_ASM", "BFLY_FWD", "BFLY_FWD_ASM", "BFLY_FWD_NC", "BFLY_FWD_NC_ASM", "BFLY_INV_ASM",
                "BFLY_INV_SCALED_ASM")


@pytest.mark.parametrize("name", list(MODS))
def test_word_serial_schedules_on_the_callers_domain(name):
    """Both restated schedules give the expected word and overflow no accumulator on every product the butterflies and the probe
    ops form -- x < 4q at q >= 2^58, x < 34q below; mred_lazy_w32 also with key words at or above q.  At the integer-class
    moduli each carry of the column form takes both values in every set, or is shown unreachable and is zero."""
    q = MODS[name]
    for op in SCHEDULE_OPS:
        if not A.applies(op, q):
            continue
        kind = A.set_kind(op)
        for x, w in A.product_operands(op, kind, q):
            want = A.w32_word(x, w, q)
            assert np.array_equal(A.w32_schedule(x, w, q), want), (op, name)
            if kind == "keys":  # the column form's domain is w < q
                keep = w < U(q)
                x, w, want = x[keep], w[keep], want[keep]
            r, carries = A.column_schedule(x, w, q)
            assert np.array_equal(r, want), (op, name)
            assert (int(x.max()) < A.lazy_bound(q)) and int(w.max()) < q
            # (the N^-1 product of the scaled butterfly has ONE second operand, the ring's constant: its carries are what they are)
            if q >= 1 << 47 and not (w == w[0]).all():
                reach = A.carries_reachable(q, A.lazy_bound(q))
                for k, (c, can) in enumerate(zip(carries, reach)):
                    assert (c.any() and not c.all()) if can else not c.any(), (op, name, f"carry {k + 1}", int(c.sum()), can)


def test_column_schedule_overflows_past_34q():
    """the middle accumulator M (x0 w1 + x1 w0, then + m q1) at the largest prime below 2^58: fits for x < 34q, overflows for
    x < 63q"""
    q = MODS["max58"]
    w = np.array([((q >> 32) - 1) << 32 | 0xFFFFFFFF], dtype=U)
    assert int(w[0]) < q
    ok = np.array([(34 * q - 1) >> 32 << 32 | 0xFFFFFFFF if ((34 * q - 1) >> 32 << 32 | 0xFFFFFFFF) < 34 * q else 34 * q - 1], dtype=U)
    A.column_schedule(ok, w, q)
    past = np.array([((63 * q - 1) >> 32) - 1 << 32 | 0xFFFFFFFF], dtype=U)
    assert 34 * q <= int(past[0]) < 63 * q
    with pytest.raises(AssertionError, match="64-bit accumulator overflow: M "):
        A.column_schedule(past, w, q)


@pytest.mark.parametrize("op,name", A.cases())
def test_expected_words_against_python_integers(op, name):
    """residue class and range map of every expected word of every set (arith_ref.check_truth).

    modmul_f64's magnitude claim |r| < 2q is asserted on |a| <= 36q: the forward row kernels hand it x[k + d], an input word
    below 2q (a lazy word; canonical and basis-extension inputs are smaller) grown by less than 2q in each of at most 17 stages
    ("34q + input", kernels.hip), and every other caller passes a residue or a sum of two products, below 4q.  On the wide set
    (|a| < 2^53) only exactness is asserted: the code does not claim the magnitude there."""
    q = MODS[name]
    for kind in A.op_sets(op):
        args, _, out0, out1 = A.reference(op, kind, q)
        A.check_truth(op, q, args, out0, out1, magnitude=A.A_MAGNITUDE * q if kind == "modmul" else None)


# ---- the header itself, on the host ---------------------------------------------------------------------------------------------
HOST_OPS = ("MRED_LAZY", "MRED", "MRED_LAZY_W32", "MRED128_LAZY", "BRED_ADD_LAZY", "BRED_ADD", "BRED_LAZY", "BRED", "MFORM_LAZY",
            "MFORM", "IMFORM_LAZY", "IMFORM")
_MAGIC = 0x4152495448303031


@pytest.fixture(scope="module")
def host_program():
    r = subprocess.run(["make", "-C", CPP, "modarith_host"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "warning" not in r.stderr, r.stderr
    return os.path.join(CPP, "modarith_host")


@pytest.mark.parametrize("name", list(MODS))
def test_modarith_header_on_the_host(host_program, name):
    q = MODS[name]
    k = A.consts(q)
    jobs, blob = [], []
    for op in HOST_OPS + ("MRED_W32",):
        ref_op = "MRED_LAZY_W32" if op == "MRED_W32" else op
        args, spans, want, _ = A.reference(ref_op, A.set_kind(ref_op), q)
        if op == "MRED_W32":
            want = A._cred(want, q)
        a = args[0]
        b = args[1] if len(args) > 1 else np.zeros_like(a)
        blob.append(np.array([_MAGIC, 13 if op == "MRED_W32" else A.OP_ID[op], q, k.qinv, k.brc0, k.brc1, len(a), 0], dtype=U).tobytes()
                    + a.tobytes() + b.tobytes())
        jobs.append((op, spans, args, want))
    r = subprocess.run([host_program], input=b"".join(blob), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    got_all = np.frombuffer(r.stdout, dtype=U)
    assert len(got_all) == sum(len(j[3]) for j in jobs)
    pos = 0
    for op, spans, args, want in jobs:
        got = got_all[pos:pos + len(want)]
        pos += len(want)
        assert np.array_equal(got, want), "host " + A.first_difference(op, name, q, spans, args, got, want)


# ---- auto_dest -------------------------------------------------------------------------------------------------------------------
def _brev32(v):
    v = ((v >> U(1)) & U(0x55555555)) | ((v & U(0x55555555)) << U(1))
    v = ((v >> U(2)) & U(0x33333333)) | ((v & U(0x33333333)) << U(2))
    v = ((v >> U(4)) & U(0x0F0F0F0F)) | ((v & U(0x0F0F0F0F)) << U(4))
    v = ((v >> U(8)) & U(0x00FF00FF)) | ((v & U(0x00FF00FF)) << U(8))
    return ((v >> U(16)) | (v << U(16))) & U(0xFFFFFFFF)


def auto_dest_model(e, ginv, logn):
    """kernels.hip auto_dest in 32-bit arithmetic"""
    sh, m32 = U(32 - logn), U(0xFFFFFFFF)
    t1 = (U(2) * (_brev32(e) >> sh) + U(1)) & m32
    t2 = ((((ginv * t1) & m32) & U((2 << logn) - 1)) - U(1) & m32) >> U(1)
    return _brev32(t2) >> sh


@pytest.mark.parametrize("logn,g", A.auto_dest_cases())
def test_auto_dest_is_the_inverse_of_the_oracles_index(logn, g):
    (e, ginv, _), dest = A.auto_dest_reference(logn, g)
    assert g % 2 == 1 and (int(ginv[0]) * g) % (2 << logn) == 1
    assert np.array_equal(auto_dest_model(e, ginv, logn), dest)


# ---- the boundary -----------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_numbered():
    import __graft_entry__ as graft
    from lattigo_amd import _lib
    graft.build()
    assert "he_debug_arith" in _lib.declared_symbols() and hasattr(_lib.load(), "he_debug_arith")
    src = open(os.path.join(ROOT, "include", "hering_debug.h")).read()
    body = re.search(r"enum he_arith_op \{(.*?)\};", src, re.S).group(1)
    names = [n.strip().split("=")[0].strip() for n in body.replace("\n", " ").split(",")]
    assert names == ["HE_ARITH_" + o for o in A.OPS] + ["HE_ARITH_COUNT"]
    ksrc = open(os.path.join(ROOT, "lattigo_amd", "csrc", "kernels.h")).read()
    kbody = re.search(r"enum ArithOp \{(.*?)\};", ksrc, re.S).group(1)
    assert [n.strip().split("=")[0].strip() for n in kbody.replace("\n", " ").split(",")] == ["ARITH_" + o for o in A.OPS] + ["ARITH_COUNT"]
