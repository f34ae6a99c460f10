"""The device compile of the scalar arithmetic primitives, one by one (`-m gpu`): he_debug_arith (include/hering_debug.h) runs the
very __device__ functions of csrc/modarith.h and csrc/kernels.hip that the production kernels call -- the hand-written
16-instruction Montgomery sequence included, which exists on the device only -- on the operand sets of tests/arith_ref.py, with
the constants of a resident ring (so q^-1, the Barrett constants, NInv and 1/q of the table builders are under test too).

Each case is one call per operand set and one exact comparison of every word with the reference that tests/test_arith_host.py
holds against Python integers without a device.  The sets sit where whole transforms do not reach: pairs of edge values, words
whose low or high 32 bits are all ones or all zero at the top of the op's domain (x < 4q at the 61-bit primes, x < 34q below
2^58), products whose low 32 / 64 bits are zero (m = 0 rounds; the documented exception of mred_lazy_w32), key words at or above
q, quotients next to a half-integer for the double-precision product, and 2^16 uniform tuples.  No tuple is skipped, filtered or
tolerated.  Moduli: one N = 2^10 ring per arithmetic class (arith_ref.moduli)."""
import ctypes as C

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd import _lib
from tests import arith_ref as A
from tests.gpu_common import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

MODS = {name: (q, c, limb) for name, q, c, limb in A.moduli()}
HE_EINVAL = -1


@pytest.fixture(scope="module")
def rings(ctx):  # noqa: F811
    return [la.Ring(ctx, A.N, A.ring_moduli(c)) for c in range(3)]


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_lib.u64p)


def debug_arith(ring, limb, op, args, pair):
    """he_debug_arith on host arrays -> (rc, out0, out1)"""
    args = [np.ascontiguousarray(a, dtype=np.uint64) for a in args] + [None] * (3 - len(args))
    n = len(args[0])
    out0 = np.full(n, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    out1 = np.full(n, 0xDEADBEEFDEADBEEF, dtype=np.uint64) if pair else None
    rc = _lib.load().he_debug_arith(ring.h, limb, op, n, _ptr(args[0]), _ptr(args[1]), _ptr(args[2]), _ptr(out0), _ptr(out1))
    return rc, out0, out1


@pytest.mark.parametrize("op,name", A.cases())
def test_primitive_on_the_device(rings, op, name):
    q, c, limb = MODS[name]
    assert rings[c].moduli[limb] == q
    for kind in A.op_sets(op):
        args, spans, want0, want1 = A.reference(op, kind, q)
        rc, got0, got1 = debug_arith(rings[c], limb, A.OP_ID[op], args, want1 is not None)
        assert rc == 0, _lib.load().he_last_error().decode()
        assert np.array_equal(got0, want0), "out0: " + A.first_difference(op, name, q, spans, args, got0, want0)
        if want1 is not None:
            assert np.array_equal(got1, want1), "out1: " + A.first_difference(op, name, q, spans, args, got1, want1)


def test_asm_form_equals_the_cpp_form_bit_for_bit(rings):
    """the hand-written sequence against mred_lazy_w32 on the same tuples, device against device, at every modulus"""
    for name, (q, c, limb) in MODS.items():
        args, spans = A.flat("w32", q)
        rc0, cpp, _ = debug_arith(rings[c], limb, A.OP_ID["MRED_LAZY_W32"], args, False)
        rc1, asm, _ = debug_arith(rings[c], limb, A.OP_ID["MRED_LAZY_ASM"], args, False)
        assert rc0 == 0 and rc1 == 0
        assert np.array_equal(asm, cpp), A.first_difference("MRED_LAZY_ASM vs MRED_LAZY_W32", name, q, spans, args, asm, cpp)
        assert (asm < np.uint64(2 * q)).all()


@pytest.mark.parametrize("logn,g", A.auto_dest_cases())
def test_auto_dest_on_the_device(rings, logn, g):
    """every e of the ring against the inverse of the oracle's AutomorphismNTTIndex"""
    args, want = A.auto_dest_reference(logn, g)
    rc, got, _ = debug_arith(rings[2], 0, A.OP_ID["AUTO_DEST"], args, False)
    assert rc == 0, _lib.load().he_last_error().decode()
    assert np.array_equal(got, want), A.first_difference("AUTO_DEST", f"logN {logn} g {g}", 2 << logn, [("all", 0, len(want))], args, got, want)


def test_resident_constants_are_the_references(rings):
    """what the probe computes with: the ring's own table against Python integers (which: 0 q, 1 qinv, 2 / 3 brc, 4 ninv)"""
    for name, (q, c, limb) in MODS.items():
        k = A.consts(q)
        assert [rings[c].constant(limb, w) for w in range(5)] == [q, k.qinv, k.brc0, k.brc1, k.ninv], name


def test_rejections(rings):
    L = _lib.load()
    a = np.arange(8, dtype=np.uint64)
    o = np.zeros(8, dtype=np.uint64)
    r, p = rings[2], _ptr

    def call(limb, op, n, a_, b_, c_, o0, o1):
        return L.he_debug_arith(r.h, limb, op, n, p(a_), p(b_), p(c_), p(o0), p(o1))

    mred, fwd, dest = A.OP_ID["MRED_LAZY"], A.OP_ID["BFLY_FWD"], A.OP_ID["AUTO_DEST"]
    assert call(0, mred, 8, a, a, None, o, None) == 0
    assert call(0, len(A.OPS), 8, a, a, a, o, o) == HE_EINVAL and b"unknown op" in L.he_last_error()
    assert call(0, -1, 8, a, a, a, o, o) == HE_EINVAL
    assert call(3, mred, 8, a, a, None, o, None) == HE_EINVAL and b"limb" in L.he_last_error()
    assert call(-1, mred, 8, a, a, None, o, None) == HE_EINVAL
    assert call(0, mred, 0, a, a, None, o, None) == HE_EINVAL
    assert call(0, mred, (1 << 20) + 1, a, a, None, o, None) == HE_EINVAL and b"2^20" in L.he_last_error()
    assert call(0, mred, 8, None, a, None, o, None) == HE_EINVAL and b"misses an array" in L.he_last_error()
    assert call(0, mred, 8, a, None, None, o, None) == HE_EINVAL
    assert call(0, mred, 8, a, a, None, None, None) == HE_EINVAL
    assert call(0, fwd, 8, a, a, None, o, o) == HE_EINVAL
    assert call(0, fwd, 8, a, a, a, o, None) == HE_EINVAL
    assert call(0, dest, 8, a, a, None, o, None) == HE_EINVAL
    assert L.he_debug_arith(C.c_uint64(0xFFFF), 0, mred, 8, p(a), p(a), None, p(o), None) != 0  # not a ring handle
    # a rejected call launches nothing and leaves the library usable; n = 2^20 is accepted (every word below q)
    big = np.arange(1 << 20, dtype=np.uint64)
    out = np.zeros(1 << 20, dtype=np.uint64)
    assert L.he_debug_arith(r.h, 0, A.OP_ID["HALVE"], 1 << 20, p(big), None, None, p(out), None) == 0
    q = np.uint64(r.moduli[0])
    assert np.array_equal(out, np.where(big & np.uint64(1), (big + q) >> np.uint64(1), big >> np.uint64(1)))
