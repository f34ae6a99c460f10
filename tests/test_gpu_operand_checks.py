"""The host-side operand checks of every entry point of tests/aliasing_table.py: one fault at a time in one polynomial parameter,
on the three rings of tests/test_gpu_aliasing.py (logN = 12 and 11, standard and conjugate-invariant), handles of batch 3 at the top
level, the submission queue off.

(a) a handle of the right shape that belongs to a second context on the same device: HE_EINVAL;
(b) a polynomial one limb short of what the level needs: HE_EINVAL (parameters that need one limb only have no such case);
(c) a batch of B + 1: HE_EINVAL.  The parameters that broadcast a batch of 1 (the inputs of he_binop and of its named forms, the
    plaintext diagonals of he_lintrans_mul_sum) take batch 1 and refuse batch 2.  he_poly_copy_batch addresses entry ranges, not
    whole batches -- a larger handle is a legal operand there: its case is a handle one entry too SMALL for the range;
(d) handle 0 and a freed handle: HE_EHANDLE.  Where the header makes the parameter optional, 0 is accepted: out2 of
    he_ckks_mul_relin with a key is no operand at all (not exercised), and ct0P[i] / ct1P[i] of he_lintrans_mul_sum are absent
    TOGETHER (the term has no P part), so the case of either passes 0 for both.

Before api.cpp declared its operands through one builder, two of the (a) cases were accepted -- the output of the he_div_* family
and of he_rescale_polys, and the vector of he_mul_by_vector_montgomery, had no context check (NOTES.md); every limb and batch
check was already there.

After the rejections of a (row, fault): every good operand downloads its pre-call words and one plain he_add on the context is
exact -- nothing was filed.  The accepted forms (broadcast, absent P part) run after that and must return 0."""
import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd._lib import load
from tests import aliasing_table as T
from tests.test_gpu_aliasing import ENVS, Case, Env, _call

pytestmark = pytest.mark.gpu

HE_EINVAL, HE_EHANDLE = -1, -2
B = 3
FAULTS = ("ctx", "limbs", "batch", "handle")
_BINOPS = ("he_binop", "he_add", "he_sub", "he_mul_coeffs_montgomery", "he_mul_coeffs_montgomery_then_add",
           "he_mul_coeffs_montgomery_lazy", "he_mul_coeffs_montgomery_lazy_then_add_lazy")
BROADCAST = {**{n: ("p1", "p2") for n in _BINOPS}, "he_lintrans_mul_sum": ("ptQ", "ptP")}


@pytest.fixture(scope="module")
def octx():
    c = la.Context(0)
    yield c
    c.sync()


@pytest.fixture(scope="module")
def envs(octx):
    return {k: Env(octx, logN, ci, 7300 + i) for i, (k, (logN, ci)) in enumerate(ENVS.items())}


@pytest.fixture(scope="module")
def other(envs):
    """a second context on the same device with the Q ring of every environment"""
    c = la.Context(0)
    yield {k: la.Ring(c, e.N, e.q, conjugate_invariant=e.ci) for k, e in envs.items()}
    c.sync()


def _operands(name):
    ops = T.operands(T.ROWS[name])
    return [o for o in ops if not (name == "he_ckks_mul_relin" and o == "out2")]  # with a key out2 is not an operand


def _needs(e, name, op, lq):
    """limbs the call needs of operand `op` at levelQ = lq, levelP = the top"""
    b = T.base(op)
    if b == "vector" or (name == "he_centered_lift" and b == "src"):
        return 1
    if (name.startswith("he_div_") or name == "he_rescale_polys") and b == "p1":
        return lq  # one division: level + 1 - nb limbs
    return lq + 1 if T.ROWS[name].side(b) == T.Q else e.np_


@pytest.mark.parametrize("fault", FAULTS)
@pytest.mark.parametrize("name", sorted(T.ROWS))
def test_operand_faults(envs, other, name, fault):
    L = load()
    for env_name, e in envs.items():
        lq = e.nq - 1
        case = Case(e, name, [], B)
        polys, good = case.distinct()
        keep, rejected, accepted = [], [], []  # (operand, what, handles of the call)

        def poly(ring, limbs, batch):
            keep.append(la.Poly(ring, limbs, batch))
            return keep[-1].h

        for op in _operands(name):
            bat = case.pre[op].shape[0]  # B (1: the vector)
            with_ = lambda h, **more: {**good, op: h, **more}
            if fault == "ctx":
                rejected.append((op, "another context", with_(poly(other[env_name], e.nq, bat)), HE_EINVAL))
            elif fault == "limbs" and _needs(e, name, op, lq) > 1:
                rejected.append((op, "one limb short", with_(poly(e.gQ, _needs(e, name, op, lq) - 1, bat)), HE_EINVAL))
            elif fault == "batch":
                if T.base(op) in BROADCAST.get(name, ()):
                    accepted.append((op, "batch 1", with_(poly(e.gQ, e.nq, 1))))
                    rejected.append((op, "batch 2", with_(poly(e.gQ, e.nq, 2)), HE_EINVAL))
                else:
                    bad = B - 1 if name == "he_poly_copy_batch" else B + 1
                    rejected.append((op, f"batch {bad}", with_(poly(e.gQ, e.nq, bad)), HE_EINVAL))
            elif fault == "handle":
                freed = la.Poly(e.gQ, e.nq, bat)
                hf = freed.h
                freed.free()
                rejected.append((op, "freed handle", with_(hf), HE_EHANDLE))
                if name == "he_lintrans_mul_sum" and T.base(op) in ("ct0P", "ct1P"):
                    twin = ("ct1P" if T.base(op) == "ct0P" else "ct0P") + op[4:]
                    accepted.append((op, "no P part", with_(0, **{twin: 0})))
                else:
                    rejected.append((op, "handle 0", with_(0), HE_EHANDLE))
        for op, what, h, want in rejected:
            rc = _call(L, e, name, h, lq, B)
            print(name, env_name, op, what, "->", rc, L.he_last_error().decode() if rc else "")
            assert rc == want, (name, env_name, op, what, rc, L.he_last_error().decode())
        e.ctx.sync()
        for op, p in polys.items():  # nothing was written ...
            assert np.array_equal(p.download(), case.pre[op]), (name, env_name, fault, op, "changed by a rejected call")
        x, y = e.words((B, e.nq, e.N)), e.words((B, e.nq, e.N))  # ... and nothing was filed: the next plain call is exact
        px, py, pz = e.poly(B, x), e.poly(B, y), e.poly(B)
        assert L.he_add(e.gQ.h, lq, px.h, py.h, pz.h) == 0
        q = np.array(e.q, dtype=np.uint64)[None, :, None]
        assert np.array_equal(pz.download(), (x + y) % q), (name, env_name, fault, "he_add after the rejections")
        for op, what, h in accepted:
            rc = _call(L, e, name, h, lq, B)
            assert rc == 0, (name, env_name, op, what, rc, L.he_last_error().decode())
        e.ctx.sync()
