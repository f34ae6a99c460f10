"""Operand identity on the device: every (entry point, aliasing pattern) of tests/aliasing_table.py, on three rings (logN = 12
with moduli of all three arithmetic classes: the fused pipelines, the NTT + MAC in doubles, giant-step fusion; logN = 11: the
separate launches; a conjugate-invariant ring at logN = 11), handles of batch 1 and 3, at the top level and one below.

Accepted patterns: every output holds, word for word, what the same call writes on distinct handles that hold the pre-call words
(the out-of-place forms are held against the oracle by the rest of the suite), and every other operand is unchanged.  Rejected
patterns: the call itself returns HE_EINVAL -- also in deferred mode -- every operand downloads byte-identical to its pre-call
contents, and the next plain call on the context is exact.  Each case runs with the submission queue off; on the logN = 12 ring
also with the queue on (four threads running the pattern on polynomials of their own beside one thread making the call without
aliasing) and in deferred mode."""
import ctypes as C
import threading

import numpy as np
import pytest

import lattigo_amd as la
from lattigo_amd._lib import H, load
from oracle import oracle as O
from oracle.circuits import _centered_lift
from tests import aliasing_table as T
from tests.helpers import rng_for

pytestmark = pytest.mark.gpu

HE_EINVAL = -1
LOGQ, LOGP = [55, 45, 58, 45], [61, 46]


class Env:
    """rings, basis extender, evaluator, a random gadget key, an index table and hoisting buffers of one configuration, on the
    device and in the oracle"""

    def __init__(self, ctx, logN, ci, seed):
        self.ctx, self.logN, self.N, self.ci = ctx, logN, 1 << logN, ci
        # moduli = 1 mod 2^13: NTT-friendly for the standard ring at logN = 12 and the conjugate-invariant one at logN = 11 (4N)
        self.q, self.p = O.GenModuli(13, LOGQ, LOGP)
        self.nq, self.np_ = len(self.q), len(self.p)
        self.gQ = la.Ring(ctx, self.N, self.q, conjugate_invariant=ci)
        self.gP = la.Ring(ctx, self.N, self.p, conjugate_invariant=ci)
        self.be = la.BasisExtender(self.gQ, self.gP)
        self.ev = la.Evaluator(self.gQ, self.gP)
        self.oQ, self.oP = O.Ring(self.N, self.q, ci), O.Ring(self.N, self.p, ci)
        self.obe, self.odc, self.oev = O.BasisExtender(self.oQ, self.oP), O.Decomposer(self.oQ, self.oP), O.Evaluator(self.oQ, self.oP)
        self.rng = rng_for(seed)
        self.bound = min(self.q + self.p)  # words below every modulus: a valid residue on either side
        beta = (self.nq + self.np_ - 1) // self.np_
        self.beta = beta
        kq = np.stack([np.stack([self.words((self.nq, self.N)) for _ in range(2)]) for _ in range(beta)])
        kp = np.stack([np.stack([self.words((self.np_, self.N)) for _ in range(2)]) for _ in range(beta)])
        self.key, self.okey = self.ev.NewEvaluationKey(kq, kp), O.EvaluationKey(kq, kp)
        self.nthroot = (4 if ci else 2) * self.N
        self.gal = pow(5, 3, self.nthroot)
        self.idx = self.gQ.AutomorphismNTTIndex(self.gal)
        self.oidx = self.oQ.AutomorphismNTTIndex(self.gal)
        self.decs, self.odecs, self.plains = {}, {}, {}

    def words(self, shape):
        return self.rng.integers(0, self.bound, size=shape, dtype=np.uint64)

    def poly(self, B, arr=None):
        p = la.Poly(self.gQ, self.nq, B)
        if arr is not None:
            p.upload(arr)
        return p

    def dec(self, B, lq):
        """the hoisting buffer of a random NTT-domain polynomial (DecomposeNTT at (lq, levelP)), on the device"""
        if (B, lq) not in self.decs:
            d = la.rlwe.Decomposition(self.ev, B)
            c2 = self.words((B, self.nq, self.N))
            self.ev.DecomposeNTT(lq, self.np_ - 1, self.np_, self.poly(B, c2), True, d)
            self.decs[(B, lq)] = d
            self.odecs[(B, lq)] = [self.oev.DecomposeNTT(lq, self.np_ - 1, self.np_, c2[b][: lq + 1], True) for b in range(B)]
        return self.decs[(B, lq)]

    def fill_dec(self, B):
        """a hoisting buffer of its own for he_decomp_fill (the ones of dec() must keep their oracle-known digits)"""
        if ("fill", B) not in self.decs:
            self.decs[("fill", B)] = la.rlwe.Decomposition(self.ev, B)
        return self.decs[("fill", B)]

    def odec(self, B, lq, b):
        self.dec(B, lq)
        return self.odecs[(B, lq)][b]


def _arr(*hs):
    return (H * len(hs))(*hs)


def _call(L, e, name, h, lq, B):
    """the entry point with operand handles h[operand]; returns the status"""
    lp, ring, be, ev, k = e.np_ - 1, e.gQ.h, e.be.h, e.ev.h, e.key.h
    u64 = lambda xs: (C.c_uint64 * len(xs))(*xs)
    sc = u64([3 + i for i in range(lq + 1)])
    if name == "he_poly_copy":
        return L.he_poly_copy(h["dst"], h["src"], lq)
    if name == "he_poly_copy_batch":
        return L.he_poly_copy_batch(h["dst"], 0, h["src"], 0, B, lq)
    if name in ("he_ntt", "he_ntt_lazy", "he_intt", "he_intt_lazy"):
        return getattr(L, name)(ring, lq, h["p1"], h["p2"])
    if name == "he_binop":
        return L.he_binop(ring, lq, 11, h["p1"], h["p2"], h["p3"])  # MulCoeffsMontgomeryThenAdd
    if name == "he_unop":
        return L.he_unop(ring, lq, 3, h["p1"], h["p2"])  # MForm
    if name == "he_scalarop":
        return L.he_scalarop(ring, lq, 3, h["p1"], 12345, h["p2"])  # MulScalarThenAdd
    if name == "he_mul_rns_scalar_montgomery":
        return L.he_mul_rns_scalar_montgomery(ring, lq, h["p1"], sc, h["p2"])
    if name.endswith("_scalar_bigint") or name == "he_mul_scalar_bigint_then_add":
        return getattr(L, name)(ring, lq, h["p1"], u64([0x123456789, 0xABCDEF]), 2, h["p2"])
    if name == "he_double_rns_scalarop":
        return L.he_double_rns_scalarop(ring, lq, 3, h["p1"], sc, u64([7 + i for i in range(lq + 1)]), h["p2"])
    if name == "he_shift":
        return L.he_shift(ring, lq, h["p1"], 5, h["p2"])
    if name == "he_mult_by_monomial":
        return L.he_mult_by_monomial(ring, lq, h["p1"], 7, h["p2"])
    if name == "he_mul_by_vector_montgomery":
        return L.he_mul_by_vector_montgomery(ring, lq, h["p1"], h["vector"], 1, h["p2"])
    if name in ("he_add", "he_sub") or name.startswith("he_mul_coeffs_montgomery"):
        return getattr(L, name)(ring, lq, h["p1"], h["p2"], h["p3"])
    if name in ("he_neg", "he_reduce", "he_mform", "he_imform"):
        return getattr(L, name)(ring, lq, h["p1"], h["p2"])
    if name.startswith("he_div_"):
        if "_many" in name:
            return getattr(L, name)(ring, lq, 1, h["p0"], h["p1"])
        return getattr(L, name)(ring, lq, h["p0"], h["p1"])
    if name == "he_rescale_polys":
        return L.he_rescale_polys(ring, lq, 1, 2, _arr(h["p0[0]"], h["p0[1]"]), _arr(h["p1[0]"], h["p1[1]"]))
    if name.startswith("he_automorphism_ntt_with_index"):
        return getattr(L, name)(ring, lq, h["pin"], e.idx.h, h["pout"])
    if name == "he_automorphism":
        return L.he_automorphism(ring, lq, h["pin"], e.gal, h["pout"])
    if name == "he_modup_q_to_p":
        return L.he_modup_q_to_p(be, lq, lp, h["polQ"], h["polP"])
    if name == "he_modup_p_to_q":
        return L.he_modup_p_to_q(be, lp, lq, h["polP"], h["polQ"])
    if name in ("he_moddown_qp_to_q", "he_moddown_qp_to_q_ntt", "he_moddown_qp_to_p"):
        return getattr(L, name)(be, lq, lp, h["p1Q"], h["p1P"], h["p2P" if name.endswith("_p") else "p2Q"])
    if name == "he_decompose_and_split":
        return L.he_decompose_and_split(ev, lq, lp, e.np_, 0, h["p0Q"], h["p1Q"], h["p1P"])
    qp4 = lambda: (h["c0Q"], h["c0P"], h["c1Q"], h["c1P"])
    if name == "he_gadget_product_lazy":
        return L.he_gadget_product_lazy(ev, lq, h["cx"], k, *qp4())
    if name == "he_gadget_product_hoisted_lazy":
        return L.he_gadget_product_hoisted_lazy(ev, lq, e.dec(B, lq).h, k, *qp4())
    if name == "he_gadget_product_hoisted_lazy_digits":
        return L.he_gadget_product_hoisted_lazy_digits(ev, lq, e.dec(B, lq).h, k, 0, (lq + 1 + lp) // (lp + 1), *qp4())
    if name == "he_moddown":
        return L.he_moddown(ev, lq, lp, *qp4(), h["out0"], h["out1"])
    if name == "he_eval_moddown_qp_to_q_ntt":
        return L.he_eval_moddown_qp_to_q_ntt(ev, lq, lp, h["p1Q"], h["p1P"], h["p2Q"])
    if name == "he_gadget_product":
        return L.he_gadget_product(ev, lq, h["cx"], k, h["out0"], h["out1"])
    if name == "he_gadget_product_hoisted":
        return L.he_gadget_product_hoisted(ev, lq, e.dec(B, lq).h, k, h["out0"], h["out1"])
    if name == "he_relinearize":
        return L.he_relinearize(ev, lq, h["in0"], h["in1"], h["in2"], k, h["out0"], h["out1"])
    if name == "he_automorphism_ct":
        return L.he_automorphism_ct(ev, lq, h["in0"], h["in1"], e.gal, k, h["out0"], h["out1"])
    if name == "he_automorphism_hoisted":
        return L.he_automorphism_hoisted(ev, lq, h["in0"], e.dec(B, lq).h, e.gal, k, h["out0"], h["out1"])
    if name == "he_automorphism_hoisted_lazy":
        return L.he_automorphism_hoisted_lazy(ev, lq, h["in0"], e.dec(B, lq).h, e.gal, k, *qp4())
    if name == "he_ckks_mul_relin":  # with the relinearization key (out2 is not an operand then)
        return L.he_ckks_mul_relin(ev, lq, h["a0"], h["a1"], h["b0"], h["b1"], k, h["out0"], h["out1"], h["out2"])
    if name == "he_bgv_mul_relin":   # without a key: the degree-2 result (out0, out1, out2)
        return L.he_bgv_mul_relin(ev, lq, 65537, h["a0"], h["a1"], h["b0"], h["b1"], 0, h["out0"], h["out1"], h["out2"])
    if name == "he_centered_lift":
        return L.he_centered_lift(ev, 0, h["src"], 1, lq, h["dstQ"], lp, h["dstP"])
    if name == "he_decomp_fill":
        return L.he_decomp_fill(e.fill_dec(B).h, lq, lp, h["srcQ"], h["srcP"])
    if name == "he_lintrans_mul_sum":
        a = lambda p: _arr(h[f"{p}[0]"], h[f"{p}[1]"])
        return L.he_lintrans_mul_sum(ev, lq, lp, 2, a("ptQ"), a("ptP"), a("ct0Q"), a("ct0P"), a("ct1Q"), a("ct1P"), _arr(e.idx.h, 0), 1,
                                     h["out0Q"], h["out0P"], h["out1Q"], h["out1P"])
    if name == "he_lintrans_giant_step":
        return L.he_lintrans_giant_step(ev, lq, h["cx"], k, e.gal, h["addQ"], h["addP"], *qp4(), 1)
    raise AssertionError(f"no call for {name}")


BIG = 0x123456789 + (0xABCDEF << 64)  # the big-integer scalar of _call
_NTT = {"he_ntt": "NTT", "he_ntt_lazy": "NTTLazy", "he_intt": "INTT", "he_intt_lazy": "INTTLazy"}
_BIN = {"he_add": "Add", "he_sub": "Sub", "he_mul_coeffs_montgomery": "MulCoeffsMontgomery",
        "he_mul_coeffs_montgomery_then_add": "MulCoeffsMontgomeryThenAdd", "he_mul_coeffs_montgomery_lazy": "MulCoeffsMontgomeryLazy",
        "he_mul_coeffs_montgomery_lazy_then_add_lazy": "MulCoeffsMontgomeryLazyThenAddLazy"}
_UN = {"he_neg": "Neg", "he_reduce": "Reduce", "he_mform": "MForm", "he_imform": "IMForm"}
_BIGINT = {"he_add_scalar_bigint": "AddScalarBigint", "he_sub_scalar_bigint": "SubScalarBigint", "he_mul_scalar_bigint": "MulScalarBigint"}
_DIV = {"he_div_round_by_last_modulus_ntt": "DivRoundByLastModulusNTT", "he_div_round_by_last_modulus": "DivRoundByLastModulus",
        "he_div_floor_by_last_modulus_ntt": "DivFloorByLastModulusNTT", "he_div_floor_by_last_modulus": "DivFloorByLastModulus",
        "he_div_round_by_last_modulus_many_ntt": "DivRoundByLastModulusManyNTT", "he_div_round_by_last_modulus_many": "DivRoundByLastModulusMany",
        "he_div_floor_by_last_modulus_many_ntt": "DivFloorByLastModulusManyNTT", "he_div_floor_by_last_modulus_many": "DivFloorByLastModulusMany"}


def _oracle(e, name, pre, B, lq):
    """The oracle's out-of-place result of _call on the pre-call words pre[operand] ([batch][nq][N] each): {written operand:
    its expected words} -- the pre-call words with the limbs the call writes replaced by the oracle's."""
    lp, L1, P1 = e.np_ - 1, lq + 1, e.np_
    oQ, oP, oev, okey, gal = e.oQ, e.oP, e.oev, e.okey, e.gal
    out = {}

    def put(op, b, rows, limb0=0):
        if op not in out:
            out[op] = pre[op].copy()
        out[op][b, limb0:limb0 + rows.shape[0]] = rows

    def putqp(names, ctQ, ctP, b):
        for k in range(2):
            put(names[2 * k], b, ctQ[k])
            put(names[2 * k + 1], b, ctP[k])

    for b in range(B):
        x = lambda op: pre[op][b if pre[op].shape[0] > 1 else 0]
        xq = lambda op: x(op)[:L1]
        xp = lambda op: x(op)[:P1]
        st = lambda *ops: np.stack([xq(o) for o in ops])
        if name in ("he_poly_copy", "he_poly_copy_batch"):
            put("dst", b, xq("src"))
        elif name in _NTT:
            put("p2", b, getattr(oQ, _NTT[name])(xq("p1")))
        elif name == "he_binop":
            put("p3", b, oQ.binop("MulCoeffsMontgomeryThenAdd", xq("p1"), xq("p2"), xq("p3")))
        elif name in _BIN:
            acc = xq("p3") if name.endswith("then_add") or name.endswith("then_add_lazy") else None
            put("p3", b, oQ.binop(_BIN[name], xq("p1"), xq("p2"), acc))
        elif name == "he_unop":
            put("p2", b, oQ.unop("MForm", xq("p1")))
        elif name in _UN:
            put("p2", b, oQ.unop(_UN[name], xq("p1")))
        elif name == "he_scalarop":
            put("p2", b, oQ.scalarop("MulScalarThenAdd", xq("p1"), 12345, xq("p2")))
        elif name == "he_mul_rns_scalar_montgomery":
            put("p2", b, oQ.MulRNSScalarMontgomery(xq("p1"), np.array([3 + i for i in range(L1)], dtype=np.uint64)))
        elif name in _BIGINT:
            put("p2", b, getattr(oQ, _BIGINT[name])(xq("p1"), BIG))
        elif name == "he_mul_scalar_bigint_then_add":
            put("p2", b, oQ.MulScalarBigintThenAdd(xq("p1"), BIG, xq("p2")))
        elif name == "he_double_rns_scalarop":
            put("p2", b, oQ.MulDoubleRNSScalarThenAdd(xq("p1"), [3 + i for i in range(L1)], [7 + i for i in range(L1)], xq("p2")))
        elif name == "he_shift":
            put("p2", b, oQ.Shift(xq("p1"), 5))
        elif name == "he_mult_by_monomial":
            put("p2", b, oQ.MultByMonomial(xq("p1"), 7))
        elif name == "he_mul_by_vector_montgomery":
            put("p2", b, oQ.MulByVectorMontgomery(xq("p1"), x("vector")[0], xq("p2")))
        elif name in _DIV:
            f = getattr(oQ, _DIV[name])
            put("p1", b, f(1, xq("p0")) if "_many" in name else f(xq("p0")))
        elif name == "he_rescale_polys":
            for i in range(T.RESCALE_N):
                put(f"p1[{i}]", b, oQ.DivRoundByLastModulusManyNTT(1, xq(f"p0[{i}]")))
        elif name == "he_automorphism_ntt_with_index":
            put("pout", b, oQ.AutomorphismNTTWithIndex(xq("pin"), e.oidx))
        elif name == "he_automorphism_ntt_with_index_then_add_lazy":
            put("pout", b, oQ.AutomorphismNTTWithIndexThenAddLazy(xq("pin"), e.oidx, xq("pout")))
        elif name == "he_automorphism":
            put("pout", b, oQ.Automorphism(xq("pin"), gal))
        elif name == "he_modup_q_to_p":
            put("polP", b, e.obe.ModUpQtoP(lq, lp, xq("polQ")))
        elif name == "he_modup_p_to_q":
            put("polQ", b, e.obe.ModUpPtoQ(lp, lq, xp("polP")))
        elif name in ("he_moddown_qp_to_q", "he_moddown_qp_to_q_ntt", "he_moddown_qp_to_p"):
            f = {"he_moddown_qp_to_q": e.obe.ModDownQPtoQ, "he_moddown_qp_to_q_ntt": e.obe.ModDownQPtoQNTT, "he_moddown_qp_to_p": e.obe.ModDownQPtoP}[name]
            put("p2P" if name.endswith("_p") else "p2Q", b, f(lq, lp, xq("p1Q"), xp("p1P")))
        elif name == "he_decompose_and_split":  # digit 0 of nbPi = P1 limbs: its own limbs are not written
            dQ, dP = e.odc.DecomposeAndSplit(lq, lp, P1, 0, xq("p0Q"))
            own = min(P1, L1)
            put("p1Q", b, dQ[own:] if own > 1 else dQ, own if own > 1 else 0)
            put("p1P", b, dP)
        elif name == "he_gadget_product_lazy":
            putqp(("c0Q", "c0P", "c1Q", "c1P"), *oev.GadgetProductLazy(lq, xq("cx"), okey), b)
        elif name in ("he_gadget_product_hoisted_lazy", "he_gadget_product_hoisted_lazy_digits"):
            putqp(("c0Q", "c0P", "c1Q", "c1P"), *oev.GadgetProductHoistedLazy(lq, *e.odec(B, lq, b), okey), b)
        elif name == "he_moddown":
            ct = oev.ModDown(lq, lp, st("c0Q", "c1Q"), np.stack([xp("c0P"), xp("c1P")]))
            put("out0", b, ct[0]); put("out1", b, ct[1])
        elif name == "he_eval_moddown_qp_to_q_ntt":
            put("p2Q", b, e.obe.ModDownQPtoQNTT(lq, lp, xq("p1Q"), xp("p1P")))
        elif name in ("he_gadget_product", "he_gadget_product_hoisted", "he_relinearize", "he_automorphism_ct", "he_automorphism_hoisted",
                      "he_ckks_mul_relin", "he_bgv_mul_relin"):
            if name == "he_gadget_product":
                ct = oev.GadgetProduct(lq, xq("cx"), okey)
            elif name == "he_gadget_product_hoisted":
                ct = oev.GadgetProductHoisted(lq, *e.odec(B, lq, b), okey)
            elif name == "he_relinearize":
                ct = oev.Relinearize(st("in0", "in1", "in2"), okey)
            elif name == "he_automorphism_ct":
                ct = oev.Automorphism(st("in0", "in1"), gal, okey)
            elif name == "he_automorphism_hoisted":
                ct = oev.AutomorphismHoisted(np.stack([xq("in0"), np.zeros_like(xq("in0"))]), *e.odec(B, lq, b), gal, okey)
            elif name == "he_ckks_mul_relin":
                ct = oev.CKKSMulRelin(st("a0", "a1"), st("b0", "b1"), okey, True)
            else:
                ct = oev.BGVMulRelin(65537, st("a0", "a1"), st("b0", "b1"), None, False)
            for k in range(ct.shape[0]):
                put(f"out{k}", b, ct[k])
        elif name == "he_automorphism_hoisted_lazy":
            putqp(("c0Q", "c0P", "c1Q", "c1P"), *oev.AutomorphismHoistedLazy(lq, xq("in0"), *e.odec(B, lq, b), gal, okey), b)
        elif name == "he_centered_lift":  # strict = 0, first_q = 1
            c = x("src")[0]
            put("dstQ", b, _centered_lift(c, e.q[0], e.q[1:L1], False), 1)
            put("dstP", b, _centered_lift(c, e.q[0], e.p, False))
        elif name == "he_decomp_fill":
            pass  # writes the hoisting buffer only
        elif name == "he_lintrans_mul_sum":  # accumulate, term 0 through the automorphism, term 1 without
            for k in range(2):
                for side, ring, rows in (("Q", oQ, L1), ("P", oP, P1)):
                    acc = x(f"out{k}{side}")[:rows]
                    for i in range(T.LINTRANS_N):
                        ct = x(f"ct{k}{side}[{i}]")[:rows]
                        if i == 0:
                            ct = ring.AutomorphismNTTWithIndex(ct, e.oidx)
                        acc = ring.binop("MulCoeffsMontgomeryThenAdd", x(f"pt{side}[{i}]")[:rows], ct, acc)
                    put(f"out{k}{side}", b, acc)
        elif name == "he_lintrans_giant_step":  # accumulate: out_k += phi(cQP_k), no reduction
            wQ, wP = oev.GadgetProductLazy(lq, xq("cx"), okey)
            for k in range(2):
                for side, ring, w, mods, rows in (("Q", oQ, wQ, e.q[:L1], L1), ("P", oP, wP, e.p, P1)):
                    v = w[k].copy()
                    if k == 0:  # ringQP.Add of canonical words
                        add = x("add" + side)[:rows]
                        for i, m in enumerate(mods):
                            t = v[i] + add[i]
                            v[i] = np.where(t >= np.uint64(m), t - np.uint64(m), t)
                    put(f"c{k}{side}", b, x(f"c{k}{side}")[:rows] + ring.AutomorphismNTTWithIndex(v, e.oidx))
        else:
            raise AssertionError(f"no oracle for {name}")
    return out


def _cases(name, B=1):
    row = T.ROWS[name]
    for groups in T.patterns(row):
        if name == "he_ckks_mul_relin" and any("out2" in g for g in groups):
            continue  # with a key out2 is not an operand of the call
        if name == "he_mul_by_vector_montgomery" and B > 1 and any("vector" in g for g in groups):
            continue  # the vector is one batch-1 polynomial: it cannot be an operand of batch B
        yield groups


class Case:
    """one aliasing pattern's handles (one per group, one per remaining operand) with random pre-call words"""

    def __init__(self, e, name, groups, B):
        self.e, self.name, self.B = e, name, B
        ops = T.operands(T.ROWS[name])
        owner = {}
        for gi, g in enumerate(groups):
            for op in g:
                owner[op] = f"g{gi}"
        self.key_of = {op: owner.get(op, op) for op in ops}
        self.keys = sorted(set(self.key_of.values()))
        bat = lambda k: 1 if any(T.base(o) == "vector" for o, kk in self.key_of.items() if kk == k) else B
        self.pre = {k: e.words((bat(k), e.nq, e.N)) for k in self.keys}
        self.ops = ops

    def handles(self):
        polys = {k: self.e.poly(self.pre[k].shape[0], self.pre[k]) for k in self.keys}
        return polys, {op: polys[self.key_of[op]].h for op in self.ops}

    def distinct(self):
        polys = {op: self.e.poly(self.pre[self.key_of[op]].shape[0], self.pre[self.key_of[op]]) for op in self.ops}
        return polys, {op: polys[op].h for op in self.ops}


LAZY = ("he_ntt_lazy", "he_intt_lazy")  # lazy outputs: words in [0, 2q) whose reduction is the oracle's (the documented contract)


def _eq(e, name, lq, got, want, written):
    if name not in LAZY or not written:
        return np.array_equal(got, want)
    q = np.array(e.q[: lq + 1], dtype=np.uint64)[None, :, None]
    g, w = got[:, : lq + 1], want[:, : lq + 1]
    return bool(np.all(g < 2 * q) and np.array_equal(g % q, w % q) and np.array_equal(got[:, lq + 1:], want[:, lq + 1:]))


def _written(case, k):
    return any(case.key_of[op] == k and T.ROWS[case.name].written(T.base(op)) for op in case.ops)


def _pre_by_op(case):
    return {op: case.pre[case.key_of[op]] for op in case.ops}


def _expected(e, case, lq):
    """the words every handle of an ACCEPTED pattern must hold afterwards: the oracle's out-of-place result on the pre-call words"""
    row = T.ROWS[case.name]
    ref = _oracle(e, case.name, _pre_by_op(case), case.B, lq)
    want = {}
    for k in case.keys:
        outs = [op for op in case.ops if case.key_of[op] == k and row.written(T.base(op)) and op in ref]
        want[k] = ref[outs[0]] if outs else case.pre[k]
    return want


def _plain(e, name, B, lq):
    """an unaliased call of the row (distinct handles) and the oracle's words for every operand: drawn once per shape"""
    if (name, B, lq) not in e.plains:
        case = Case(e, name, [], B)
        ref = _oracle(e, name, _pre_by_op(case), B, lq)
        e.plains[(name, B, lq)] = (case, {op: ref.get(op, case.pre[op]) for op in case.ops})
    return e.plains[(name, B, lq)]


def _check_plain(L, e, name, B, lq, tag, polys=None, rc=None):
    """run (or check an already-run) unaliased call against the oracle"""
    case, want = _plain(e, name, B, lq)
    if polys is None:
        polys, h = case.distinct()
        rc = _call(L, e, name, h, lq, B)
        e.ctx.sync()
    assert rc == 0, (tag, "plain call", load().he_last_error().decode())
    for op, p in polys.items():
        assert _eq(e, name, lq, p.download(), want[op], T.ROWS[name].written(T.base(op))), (tag, "plain call", op)


def _run_case(L, e, name, groups, B, lq, mode):
    """one pattern: accepted -> every handle holds the oracle's words; rejected -> HE_EINVAL at once, nothing changed, and an
    unaliased call right after it (still in the same mode) matches the oracle"""
    row = T.ROWS[name]
    accept = T.pattern_verdict(row, groups) == "accept"
    case = Case(e, name, groups, B)
    want = _expected(e, case, lq) if accept else case.pre
    tag = (name, T.pattern_id(groups), B, lq, mode)
    ctx = e.ctx
    if mode == "queue":  # four callers with the pattern on handles of their own, one unaliased caller beside them
        ctx.SetCoalescing(16, 3000)
        try:
            mine = [case.handles() for _ in range(4)]
            pcase, _ = _plain(e, name, B, lq)
            plain = pcase.distinct()
            rcs, errs = [None] * 5, [None] * 5
            bar = threading.Barrier(5)

            def work(i):
                bar.wait()
                h = mine[i][1] if i < 4 else plain[1]
                rcs[i] = _call(L, e, name, h, lq, B)
                errs[i] = load().he_last_error().decode()

            ts = [threading.Thread(target=work, args=(i,)) for i in range(5)]
            for t in ts:
                t.start()
            for t in ts:
                t.join()
            ctx.sync()
            for i in range(4):
                assert rcs[i] == (0 if accept else HE_EINVAL), (tag, i, rcs[i], errs[i])
                for k, p in mine[i][0].items():
                    assert _eq(e, name, lq, p.download(), want[k], accept and _written(case, k)), (tag, i, k)
            _check_plain(L, e, name, B, lq, tag, plain[0], rcs[4])
            if not accept:  # the queue is still usable after the rejections
                _check_plain(L, e, name, B, lq, tag)
        finally:
            ctx.SetCoalescing(0, 0)
        return
    polys, h = case.handles()
    if mode == "deferred":
        ctx.SetCoalescing(16, 3000)
        ctx.SetDeferred(4)
    try:
        rc = _call(L, e, name, h, lq, B)
        err = load().he_last_error().decode()
        ctx.sync()
        assert rc == (0 if accept else HE_EINVAL), (tag, rc, err)
        for k, p in polys.items():
            assert _eq(e, name, lq, p.download(), want[k], accept and _written(case, k)), (tag, k)
        if not accept:  # the context -- in deferred mode its queue -- is still usable: a plain call after the rejection is exact
            _check_plain(L, e, name, B, lq, tag)
    finally:
        if mode == "deferred":
            ctx.SetDeferred(0)
            ctx.SetCoalescing(0, 0)


ENVS = {"std12": (12, False), "std11": (11, False), "ci11": (11, True)}


@pytest.fixture(scope="module")
def actx():
    c = la.Context(0)
    yield c
    c.sync()


@pytest.fixture(scope="module")
def envs(actx):
    return {k: Env(actx, logN, ci, 7100 + i) for i, (k, (logN, ci)) in enumerate(ENVS.items())}


MODES = ["off", "queue", "deferred"]
BATCHES = (1, 3)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(T.ROWS))
def test_aliasing_patterns(envs, name, mode):
    """every pattern of the row on the three rings x batch 1, 3 x the top level and one below, with the submission queue off,
    on (four aliasing callers beside one unaliased caller) and deferred.  Queued: the four aliasing callers' requests form
    batches of their own, never one batch with the unaliased caller's request (a different aliasing pattern is a different key)."""
    L = load()
    rpc = T.RESCALE_N if name == "he_rescale_polys" else 1  # requests filed per call
    for env_name, e in envs.items():
        for B in BATCHES:
            for lq in (e.nq - 1, e.nq - 2):
                for groups in _cases(name, B):
                    before = e.ctx.CoalescingStats()
                    _run_case(L, e, name, groups, B, lq, mode)
                    after = e.ctx.CoalescingStats()
                    dc, dl = after["calls"] - before["calls"], after["launches"] - before["launches"]
                    # (he_rescale_polys files one request per pair: inputs shared BETWEEN pairs are no request's pattern -- both
                    # only read them, so such requests batch with the unaliased caller's, legitimately)
                    cross = name == "he_rescale_polys" and any(len({o[-2] for o in g}) > 1 for g in groups)
                    if mode == "queue" and not cross and T.pattern_verdict(T.ROWS[name], groups) == "accept" and dc >= 5 * rpc:
                        assert dl >= 2, (name, T.pattern_id(groups), env_name, B, lq, "aliased and unaliased requests in one launch")


def test_copy_batch_ranges_of_one_handle(envs):
    """he_poly_copy_batch within one handle: disjoint entry ranges copy, overlapping ones are rejected and change nothing"""
    L = load()
    e = envs["std12"]
    x = e.words((3, e.nq, e.N))
    p = e.poly(3, x)
    assert L.he_poly_copy_batch(p.h, 2, p.h, 0, 1, e.nq - 1) == 0
    want = x.copy()
    want[2] = x[0]
    assert np.array_equal(p.download(), want)
    for dst_b0, src_b0, nb in ((1, 0, 2), (0, 1, 2), (0, 0, 3)):
        assert L.he_poly_copy_batch(p.h, dst_b0, p.h, src_b0, nb, e.nq - 1) == HE_EINVAL
        e.ctx.sync()
        assert np.array_equal(p.download(), want)


@pytest.mark.parametrize("env_name", list(ENVS))
def test_galois_elements_act_mod_nthroot(envs, env_name):
    """any odd g gives the words of g mod NthRoot (2N, 4N on conjugate-invariant rings): g + NthRoot k with values past 2^32,
    and 2^64 - 1 (conjugation) -- ring automorphisms, index tables, Automorphism on ciphertexts and the giant step"""
    L = load()
    e = envs[env_name]
    lq, lp, B = e.nq - 1, e.np_ - 1, 1
    for g in (e.gal, e.nthroot - 1):
        bigs = [g + e.nthroot * (1 << 33)] + ([(1 << 64) - 1] if g == e.nthroot - 1 else [])
        for big in bigs:
            assert big % e.nthroot == g and big >= 1 << 32
            ia, ib = la.ring.AutomorphismIndex(e.gQ, g), la.ring.AutomorphismIndex(e.gQ, big)
            assert np.array_equal(ia.download(), ib.download()), (g, big)
            x = [e.poly(B, e.words((B, e.nq, e.N))) for _ in range(4)]
            outs = {}
            for gg in (g, big):
                o = [e.poly(B) for _ in range(3)]
                assert L.he_automorphism(e.gQ.h, lq, x[0].h, gg, o[0].h) == 0
                assert L.he_automorphism_ct(e.ev.h, lq, x[0].h, x[1].h, gg, e.key.h, o[1].h, o[2].h) == 0
                outs[gg] = o
            e.ctx.sync()
            for i in range(3):
                assert np.array_equal(outs[g][i].download(), outs[big][i].download()), (g, big, i)
            # the giant step, overwriting (fresh accumulators for both elements)
            res = {}
            for gg in (g, big):
                o = [e.poly(B) for _ in range(4)]
                assert L.he_lintrans_giant_step(e.ev.h, lq, x[2].h, e.key.h, gg, x[3].h, x[1].h, *[p.h for p in o], 0) == 0
                res[gg] = [p.download() for p in o]
            for a, b in zip(res[g], res[big]):
                assert np.array_equal(a, b), (g, big)
            # the same element through the queue: g and g + k NthRoot requests share a batch key
            e.ctx.SetCoalescing(16, 3000)
            try:
                o = [[e.poly(B) for _ in range(2)] for _ in range(2)]
                rcs = [None, None]
                bar = threading.Barrier(2)

                def work(i, gg):
                    bar.wait()
                    rcs[i] = L.he_automorphism_ct(e.ev.h, lq, x[0].h, x[1].h, gg, e.key.h, o[i][0].h, o[i][1].h)

                ts = [threading.Thread(target=work, args=(i, gg)) for i, gg in enumerate((g, big))]
                for t in ts:
                    t.start()
                for t in ts:
                    t.join()
                e.ctx.sync()
            finally:
                e.ctx.SetCoalescing(0, 0)
            assert rcs == [0, 0]
            for i in range(2):
                for c in range(2):
                    assert np.array_equal(o[i][c].download(), outs[g][1 + c].download()), (g, big, i, c)
