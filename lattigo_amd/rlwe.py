"""Host-side mirror of the rlwe.Evaluator hot path (core/rlwe/evaluator*.go,
operator interface core/rlwe/rlwe.go:10-18) and of the CKKS/BGV call sites that
sit on it, backed by libhering's HIP kernels.  NTT-domain ciphertexts; a
ciphertext is a list of ``Poly`` (rlwe.Ciphertext.Value), a QP element a
``(Q, P)`` pair of ``Poly`` (ringqp.Poly)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import H, HeringError, check, load, u64p
from .ring import BasisExtender, Poly, Ring, _p


def BaseRNSDecompositionVectorSize(levelQ: int, levelP: int) -> int:
    """core/rlwe/params.go:543-550"""
    if levelP == -1:
        return levelQ + 1
    return (levelQ + levelP + 1) // (levelP + 1)


class EvaluationKey:
    """rlwe.GadgetCiphertext / EvaluationKey with BaseTwoDecomposition = 0
    (core/rlwe/gadgetciphertext.go:19): q [beta,2,nQk,N], p [beta,2,nPk,N], NTT + Montgomery."""

    def __init__(self, evaluator: "Evaluator", q: np.ndarray, p: np.ndarray, BaseTwoDecomposition: int = 0,
                 BaseTwoDecompositionVectorSize=None, shape=None):
        if shape is not None:  # (beta, nQk, nPk): a zeroed key to be filled on the device (DeviceBuffer / Commit)
            self.beta, self.nQk, self.nPk = shape
            q = p = None
        else:
            q = np.ascontiguousarray(q, dtype=np.uint64)
            # p = None: a key without P part (parameters without special primes, levelP = -1; base-2 gadgets only)
            p = np.zeros(q.shape[:2] + (0, q.shape[3]), dtype=np.uint64) if p is None else np.ascontiguousarray(p, dtype=np.uint64)
            assert q.ndim == 4 and p.ndim == 4 and q.shape[:2] == p.shape[:2] and q.shape[1] == 2
            self.beta, self.nQk, self.nPk = q.shape[0], q.shape[2], p.shape[2]
        self.N = evaluator.ringQ.N
        self.BaseTwoDecomposition = BaseTwoDecomposition
        self.BaseTwoDecompositionVectorSize = list(BaseTwoDecompositionVectorSize) if BaseTwoDecomposition else None
        h = H()
        pq, pp = (None, None) if q is None else (_p(q), _p(p) if p.size else None)
        if BaseTwoDecomposition:
            nj = (C.c_int * len(BaseTwoDecompositionVectorSize))(*BaseTwoDecompositionVectorSize)
            check(load().he_evk_create_base2(evaluator.h, BaseTwoDecomposition, nj, len(BaseTwoDecompositionVectorSize),
                                             self.nQk, self.nPk, pq, pp, C.byref(h)))
        else:
            check(load().he_evk_create(evaluator.h, self.beta, self.nQk, self.nPk, pq, pp, C.byref(h)))
        self.h = h.value

    def LevelQ(self):
        return self.nQk - 1

    def LevelP(self):
        return self.nPk - 1

    def Shape(self):
        """What a peer needs to allocate the same key: (beta, nQk, nPk, BaseTwoDecomposition, vector sizes)."""
        return (self.beta, self.nQk, self.nPk, self.BaseTwoDecomposition, self.BaseTwoDecompositionVectorSize)

    def DeviceBuffer(self):
        """(device pointer, bytes) of the key words [beta][2][nQk + nPk][N]; the context's stream is drained first."""
        ptr, nb = C.c_void_p(), C.c_size_t()
        check(load().he_evk_device_buffer(self.h, C.byref(ptr), C.byref(nb)))
        return ptr.value, nb.value

    def Commit(self):
        """After an external device-side write of the key words (RCCL broadcast) has completed."""
        check(load().he_evk_commit(self.h))

    def download(self) -> np.ndarray:
        """The key words as [beta, 2, nQk + nPk, N] (tests / wire export)."""
        out = np.empty((self.beta, 2, self.nQk + self.nPk, self.N), dtype=np.uint64)
        check(load().he_evk_download(self.h, _p(out), out.size))
        return out

    def __del__(self):
        try:
            if getattr(self, "h", None):
                load().he_evk_destroy(self.h)
                self.h = None
        except Exception:
            pass


class Decomposition:
    """BuffDecompQP []ringqp.Poly of Evaluator.DecomposeNTT, device resident."""

    def __init__(self, evaluator: "Evaluator", batch: int = 1):
        self.ev = evaluator
        self.batch = batch
        h = H()
        check(load().he_decomp_create(evaluator.h, batch, C.byref(h)))
        self.h = h.value

    def limb(self, b, digit, is_p, limb) -> np.ndarray:
        out = np.empty(self.ev.ringQ.N, dtype=np.uint64)
        check(load().he_decomp_download_limb(self.h, b, digit, int(is_p), limb, _p(out)))
        return out

    def __del__(self):
        try:
            if getattr(self, "h", None):
                load().he_decomp_destroy(self.h)
                self.h = None
        except Exception:
            pass


class Evaluator:
    """rlwe.Evaluator (core/rlwe/evaluator.go:12) restricted to the key-switch path."""

    def __init__(self, ringQ: Ring, ringP: Ring | None):
        """ringP = None: parameters without special primes (rlwe.ParametersLiteral.P = nil): levelP = -1 in every call, keys
        are base-2 gadgets without a P part and a QP element is a (Q, None) pair."""
        self.ringQ, self.ringP = ringQ, ringP
        h = H()
        check(load().he_evaluator_create(ringQ.h, ringP.h if ringP is not None else 0, C.byref(h)))
        self.h = h.value

    def __del__(self):
        try:
            if getattr(self, "h", None):
                load().he_evaluator_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def NewEvaluationKey(self, q, p, BaseTwoDecomposition=0, BaseTwoDecompositionVectorSize=None) -> EvaluationKey:
        return EvaluationKey(self, q, p, BaseTwoDecomposition, BaseTwoDecompositionVectorSize)

    def SetCoalescing(self, max_batch: int = 64, window_us: int = 30):
        """he_evaluator_set_coalescing (include/hering.h): concurrent single-ciphertext MulRelin calls on this evaluator -- one
        OS thread per ciphertext, the reference's own parallel mode (b.RunParallel over shallow copies of one evaluator,
        schemes/ckks/ckks_benchmarks_test.go:116-207, core/rlwe/evaluator.go:200-227) -- are gathered into batched launches
        over the callers' own polynomials.  max_batch <= 1 switches it off."""
        check(load().he_evaluator_set_coalescing(self.h, max_batch, window_us))

    def CoalescingStats(self) -> dict:
        out = (C.c_uint64 * 4)()
        check(load().he_evaluator_coalescing_stats(self.h, out))
        return {"calls": int(out[0]), "launches": int(out[1]), "largest_batch": int(out[2]), "one_by_one": int(out[3])}

    def EvaluationKeyFromBinary(self, data: bytes) -> EvaluationKey:
        """rlwe.EvaluationKey.UnmarshalBinary (core/rlwe/keys.go:443 -> gadgetciphertext.go:134): load a key the
        reference serialised straight into a device handle."""
        from . import wire
        kq, kp, base_two, nj = wire.gadget_ciphertext_unmarshal(data)
        return EvaluationKey(self, kq, kp, base_two, nj if base_two else None)

    def GaloisKeyFromBinary(self, data: bytes):
        """rlwe.GaloisKey.UnmarshalBinary (core/rlwe/keys.go:659) -> (GaloisElement, NthRoot, EvaluationKey)"""
        from . import wire
        g, nth, kq, kp, base_two, nj = wire.galois_key_unmarshal(data)
        return g, nth, EvaluationKey(self, kq, kp, base_two, nj if base_two else None)

    # ring.Decomposer.DecomposeAndSplit (ring/basis_extension.go:381)
    def DecomposeAndSplit(self, levelQ, levelP, nbPi, digit, p0Q: Poly, p1Q: Poly, p1P: Poly):
        check(load().he_decompose_and_split(self.h, levelQ, levelP, nbPi, digit, p0Q.h, p1Q.h, p1P.h))

    # EvaluatorProvider.DecomposeNTT (core/rlwe/evaluator_gadget_product.go:459)
    def DecomposeNTT(self, levelQ, levelP, nbPi, c2: Poly, c2IsNTT: bool, decomp: Decomposition):
        check(load().he_decompose_ntt(self.h, levelQ, levelP, nbPi, c2.h, int(c2IsNTT), decomp.h))

    # EvaluatorProvider.GadgetProductLazy (:108); ctQP = [(Q0,P0),(Q1,P1)].  isNTT is the IsNTT flag of ctQP, i.e. the
    # domain of cx and of the result (:121-125, :142-152)
    def GadgetProductLazy(self, levelQ, cx: Poly, evk: EvaluationKey, ctQP, isNTT: bool = True):
        (q0, p0), (q1, p1) = ctQP
        hp = lambda p: p.h if p is not None else 0  # levelP = -1: no P part
        if isNTT:
            check(load().he_gadget_product_lazy(self.h, levelQ, cx.h, evk.h, q0.h, hp(p0), q1.h, hp(p1)))
            return
        rQ = self.ringQ.AtLevel(levelQ)
        rP = self.ringP.AtLevel(evk.LevelP()) if evk.LevelP() >= 0 else None
        cxNTT = Poly(self.ringQ, levelQ + 1, cx.batch, zero=False)
        rQ.NTT(cx, cxNTT)
        check(load().he_gadget_product_lazy(self.h, levelQ, cxNTT.h, evk.h, q0.h, hp(p0), q1.h, hp(p1)))
        for q, p in ctQP:  # ringQP.INTT (:121-125)
            rQ.INTT(q, q)
            if rP is not None:
                rP.INTT(p, p)

    # EvaluatorProvider.GadgetProductHoistedLazy (:379)
    def GadgetProductHoistedLazy(self, levelQ, decomp: Decomposition, evk: EvaluationKey, ctQP):
        (q0, p0), (q1, p1) = ctQP
        check(load().he_gadget_product_hoisted_lazy(self.h, levelQ, decomp.h, evk.h, q0.h, p0.h, q1.h, p1.h))

    def GadgetProductHoistedLazyDigits(self, levelQ, decomp: Decomposition, evk: EvaluationKey, digit_begin: int, digit_end: int, ctQP):
        """the inner product of GadgetProductHoistedLazy over the digits [digit_begin, digit_end) only (canonical): the
        per-rank share when one key switch is split over several GPUs by digit (dist.SplitGadgetProductHoisted)"""
        (q0, p0), (q1, p1) = ctQP
        check(load().he_gadget_product_hoisted_lazy_digits(self.h, levelQ, decomp.h, evk.h, digit_begin, digit_end, q0.h, p0.h, q1.h, p1.h))

    # Evaluator.ModDown (:39-97), the four domain combinations of (ctQP.IsNTT, ct.IsNTT); ctQP is modified in place in the
    # NTT -> INTT case, as the reference
    # BasisExtender.ModDownQPtoQNTT (ring/basis_extension.go:235) on the evaluator's fused pipeline; p2Q may alias p1Q
    def ModDownQPtoQNTT(self, levelQ, levelP, p1Q: Poly, p1P: Poly, p2Q: Poly):
        check(load().he_eval_moddown_qp_to_q_ntt(self.h, levelQ, levelP, p1Q.h, p1P.h, p2Q.h))

    def ModDown(self, levelQ, levelP, ctQP, ct, ctQPIsNTT: bool = True, ctIsNTT: bool = True):
        (q0, p0), (q1, p1) = ctQP
        if levelP == -1:  # no special primes (:74-96): a copy, or one NTT / INTT of the Q part
            rQ = self.ringQ.AtLevel(levelQ)
            if ctQPIsNTT == ctIsNTT:
                check(load().he_moddown(self.h, levelQ, -1, q0.h, 0, q1.h, 0, ct[0].h, ct[1].h))
            else:
                for q, o in zip((q0, q1), ct):
                    (rQ.INTT if ctQPIsNTT else rQ.NTT)(q, o)
            return
        if ctQPIsNTT and ctIsNTT:
            check(load().he_moddown(self.h, levelQ, levelP, q0.h, p0.h, q1.h, p1.h, ct[0].h, ct[1].h))
            return
        from .ring import BasisExtender
        if getattr(self, "_be", None) is None:
            self._be = BasisExtender(self.ringQ, self.ringP)
        rQ, rP = self.ringQ.AtLevel(levelQ), self.ringP.AtLevel(levelP)
        if ctQPIsNTT:  # NTT -> INTT (:51-58)
            for q, p in ctQP:
                rQ.INTTLazy(q, q)
                rP.INTTLazy(p, p)
        for (q, p), o in zip(ctQP, ct):
            self._be.ModDownQPtoQ(levelQ, levelP, q, p, o)
        if not ctQPIsNTT and ctIsNTT:  # INTT -> NTT (:62-67)
            for o in ct:
                rQ.NTT(o, o)

    # Evaluator.GadgetProduct (:16) / GadgetProductHoisted (:348); isNTT = ct.IsNTT (domain of cx and of the result)
    def GadgetProduct(self, levelQ, cx: Poly, evk: EvaluationKey, ct, isNTT: bool = True):
        if isNTT:
            check(load().he_gadget_product(self.h, levelQ, cx.h, evk.h, ct[0].h, ct[1].h))
            return
        B = cx.batch
        ctQP = [(Poly(self.ringQ, levelQ + 1, B, zero=False),
                 Poly(self.ringP, evk.LevelP() + 1, B, zero=False) if evk.LevelP() >= 0 else None) for _ in range(2)]
        self.GadgetProductLazy(levelQ, cx, evk, ctQP, isNTT=False)
        self.ModDown(levelQ, evk.LevelP(), ctQP, ct, ctQPIsNTT=False, ctIsNTT=False)

    def GadgetProductHoisted(self, levelQ, decomp: Decomposition, evk: EvaluationKey, ct):
        check(load().he_gadget_product_hoisted(self.h, levelQ, decomp.h, evk.h, ct[0].h, ct[1].h))

    # Evaluator.ApplyEvaluationKey (core/rlwe/evaluator_evaluationkey.go:36-106): ctIn and opOut of the evaluator's degree, or
    # one of them of a smaller degree n (the key then switches between the secret of degree N and the small secret mapped up);
    # isNTT = ctIn.IsNTT.  The coefficient-domain form is composed here from the NTT-domain call, as GadgetProduct(isNTT=False).
    def ApplyEvaluationKey(self, level, ctIn, evk: EvaluationKey, opOut, isNTT: bool = True):
        if isNTT:
            check(load().he_apply_evaluation_key(self.h, level, ctIn[0].h, ctIn[1].h, evk.h, opOut[0].h, opOut[1].h))
            return
        N, NIn, NOut = self.ringQ.N, ctIn[0].N, opOut[0].N
        if max(NIn, NOut) != N:  # (:51-53, :68-70; the same degree must be the evaluator's as well)
            raise HeringError(-1, "cannot ApplyEvaluationKey: the large side's ring degree does not match evaluator params ring degree")
        level = min(level, evk.LevelQ())
        rQ = self.ringQ.AtLevel(level)
        B = ctIn[0].batch
        if NIn < NOut:  # SwitchCiphertextRingDegree into opOut (:56-58), then the key switch on opOut in place
            SwitchCiphertextRingDegree(ctIn, opOut)
            ctIn = opOut
        t = [Poly(self.ringQ, level + 1, B, zero=False) for _ in range(2)]
        for c, d in zip(ctIn, t):
            rQ.NTT(c, d)
        u = opOut if NIn <= NOut else [Poly(self.ringQ, level + 1, B, zero=False) for _ in range(2)]
        check(load().he_apply_evaluation_key(self.h, level, t[0].h, t[1].h, evk.h, u[0].h, u[1].h))
        for c in u:
            rQ.INTT(c, c)
        if NIn > NOut:  # SwitchCiphertextRingDegree of the key-switched ciphertext (:85-87)
            SwitchCiphertextRingDegree(u, opOut)

    # Evaluator.Relinearize (core/rlwe/evaluator_evaluationkey.go:117)
    def Relinearize(self, level, ctIn, rlk: EvaluationKey, opOut):
        check(load().he_relinearize(self.h, level, ctIn[0].h, ctIn[1].h, ctIn[2].h, rlk.h, opOut[0].h, opOut[1].h))

    # Evaluator.Automorphism (core/rlwe/evaluator_automorphism.go:13)
    def Automorphism(self, level, ctIn, galEl: int, gk: EvaluationKey, opOut):
        check(load().he_automorphism_ct(self.h, level, ctIn[0].h, ctIn[1].h, galEl, gk.h, opOut[0].h, opOut[1].h))

    # Evaluator.AutomorphismHoisted (:60)
    def AutomorphismHoisted(self, level, ctIn, c1DecompQP: Decomposition, galEl: int, gk: EvaluationKey, opOut):
        check(load().he_automorphism_hoisted(self.h, level, ctIn[0].h, c1DecompQP.h, galEl, gk.h, opOut[0].h, opOut[1].h))

    # EvaluatorProvider.AutomorphismHoistedLazy (:104)
    def AutomorphismHoistedLazy(self, levelQ, ctIn, c1DecompQP: Decomposition, galEl: int, gk: EvaluationKey, ctQP):
        (q0, p0), (q1, p1) = ctQP
        check(load().he_automorphism_hoisted_lazy(self.h, levelQ, ctIn[0].h, c1DecompQP.h, galEl, gk.h,
                                                  q0.h, p0.h, q1.h, p1.h))

    # the giant step of lintrans.Evaluator.MultiplyByDiagMatrixBSGS (circuits/common/lintrans/lintrans_evaluator.go:397-441):
    # GadgetProductLazy(cx) -> cQP; cQP[0] += addQP; outQP[k] (+)= phi_galEl(cQP[k]) -- he_lintrans_giant_step
    def LinTransGiantStep(self, levelQ, cx: Poly, gk: EvaluationKey, galEl: int, addQP, outQP, accumulate: bool):
        (q0, p0), (q1, p1) = outQP
        check(load().he_lintrans_giant_step(self.h, levelQ, cx.h, gk.h, galEl, addQP[0].h, addQP[1].h, q0.h, p0.h, q1.h, p1.h,
                                            1 if accumulate else 0))

    # schemes/ckks Evaluator.Mul / MulRelin (schemes/ckks/evaluator.go:613,742 -> mulRelin :764)
    def CKKSMulRelin(self, level, op0, op1, rlk: EvaluationKey | None, opOut):
        o2 = opOut[2].h if rlk is None else 0
        check(load().he_ckks_mul_relin(self.h, level, op0[0].h, op0[1].h, op1[0].h, op1[1].h, rlk.h if rlk else 0,
                                       opOut[0].h, opOut[1].h, o2))

    # schemes/bgv Evaluator.Mul / MulRelin (schemes/bgv/evaluator.go:529 -> tensorStandard :592)
    def BGVMulRelin(self, level, t: int, op0, op1, rlk: EvaluationKey | None, opOut):
        o2 = opOut[2].h if rlk is None else 0
        check(load().he_bgv_mul_relin(self.h, level, t, op0[0].h, op0[1].h, op1[0].h, op1[1].h, rlk.h if rlk else 0,
                                      opOut[0].h, opOut[1].h, o2))

    # schemes/{ckks,bgv} Evaluator.Rescale (ckks :477, bgv :1363)
    def Rescale(self, level, nbRescales, op0, opOut):
        n = min(len(op0), len(opOut))
        hs = lambda ps: (H * n)(*[p.h for p in ps[:n]])
        check(load().he_rescale_polys(self.ringQ.h, level, nbRescales, n, hs(op0), hs(opOut)))


# ----------------------------------------------------------------------------------------------------
# core/rlwe/inner_sum.go: Trace / PartialTracesSum / InnerSum / Replicate.  Host-side drivers over the
# device-resident operators above, exactly as the reference's own code sits on rlwe.EvaluatorProvider.
# ----------------------------------------------------------------------------------------------------
GaloisGen = 5  # core/rlwe/params.go:33


# rlwe.SwitchCiphertextRingDegreeNTT (core/rlwe/element.go:250): ctIn, opOut lists of Poly (rlwe.Element.Value); ringQLargeDim
# is required for large -> small (its moduli are those of the small polynomials' limbs) and may be None otherwise
def SwitchCiphertextRingDegreeNTT(ctIn, ringQLargeDim: Ring | None, opOut):
    for a, b in zip(ctIn, opOut):
        check(load().he_switch_ring_degree_ntt(ringQLargeDim.h if ringQLargeDim is not None else 0, min(a.Level(), b.Level()), a.h, b.h))


# rlwe.SwitchCiphertextRingDegree (core/rlwe/element.go:293), coefficient domain: up leaves the words of opOut between the
# multiples of gap untouched, as the reference
def SwitchCiphertextRingDegree(ctIn, opOut):
    for a, b in zip(ctIn, opOut):
        check(load().he_switch_ring_degree(min(a.Level(), b.Level()), a.h, b.h))


def GaloisElement(nth_root: int, k: int) -> int:
    """Parameters.GaloisElement (core/rlwe/params.go:580): GaloisGen^k mod NthRoot, k reduced as a uint64."""
    return pow(GaloisGen, (k & 0xFFFFFFFFFFFFFFFF) & (nth_root - 1), nth_root)


class GaloisKeySet:
    """rlwe.MemEvaluationKeySet restricted to Galois keys (core/rlwe/evaluationkeyset.go): galEl -> EvaluationKey."""

    def __init__(self, keys: dict | None = None):
        self.keys = dict(keys or {})

    def GetGaloisKey(self, galEl: int) -> EvaluationKey:
        if galEl not in self.keys:
            raise KeyError(f"GaloisKey[{galEl}] is nil")
        return self.keys[galEl]


# ---- the ring-packing evaluator (core/rlwe/ring_packing.go; include/hering_ringpack.h) -------------------------------------------
def GaloisElementsForExpand(nth_root: int, logN: int):
    """rlwe.GaloisElementsForExpand (core/rlwe/ring_packing_keys.go:143)"""
    return [nth_root // (2 << i) + 1 for i in range(logN)]


def GaloisElementsForPack(nth_root: int, logN_ring: int, logGap: int):
    """rlwe.GaloisElementsForPack (core/rlwe/ring_packing_keys.go:156), standard ring"""
    if logGap > logN_ring or logGap < 0:
        raise ValueError("cannot GaloisElementsForPack: logGap > logN || logGap < 0")
    galEls = [GaloisElement(nth_root, 1 << i) for i in range(logGap)]
    if logGap == logN_ring:
        galEls.append(nth_root - 1)  # GaloisElementOrderTwoOrthogonalSubgroup
    return galEls


def getMinimumGap(lst):
    """core/rlwe/ring_packing.go:812: (the odd part of the smallest gap, log2 of its power-of-two part) of a sorted index list"""
    gap, logGap = 0x7FFFFFFFFFFFFFFF, 0
    for a, b in zip(lst, lst[1:]):
        if a > b:
            raise ValueError("invalid index list: element must be sorted from smallest to largest")
        if a == b:
            raise ValueError("invalid index list: contains duplicated elements")
        gap = min(gap, b - a)
        if gap == 1:
            break
    while gap & 1 == 0:
        logGap += 1
        gap >>= 1
    return gap, logGap


def XPow2NTT(ring: Ring, level: int, i: int, div: bool, out: Poly):
    """GenXPow2NTT(ring.AtLevel(level), logN, div)[i] (core/rlwe/ring_packing.go:772), read off the resident twiddle tables"""
    check(load().he_ring_xpow2_ntt(ring.h, level, i, int(div), out.h))


def SplitNTT(ringLarge: Ring, level: int, pIn: Poly, outEven: Poly, outOdd: Poly | None = None):
    """the ring maps of Split (core/rlwe/ring_packing.go:205-225) on one polynomial"""
    check(load().he_ring_split_ntt(ringLarge.h, level, pIn.h, outEven.h, outOdd.h if outOdd is not None else 0))


def MergeNTT(ringLarge: Ring, level: int, inEven: Poly, inOdd: Poly | None, out: Poly):
    """the ring maps of Merge (core/rlwe/ring_packing.go:410-417) on one polynomial"""
    check(load().he_ring_merge_ntt(ringLarge.h, level, inEven.h, inOdd.h if inOdd is not None else 0, out.h))


def _harr(polys):
    return (H * len(polys))(*[p.h if p is not None else 0 for p in polys])


class RingPackingEvaluator:
    """rlwe.RingPackingEvaluator (core/rlwe/ring_packing.go:13) on device-resident ciphertexts.

    Evaluators: {logN: Evaluator} (rings of the same moduli at every degree); RingSwitchingKeys: {(logN_from, logN_to):
    EvaluationKey of the evaluator of the larger degree}; RepackKeys / ExtractKeys: {logN: GaloisKeySet}.  Ciphertexts are
    [Poly, Poly] in the NTT domain unless isNTT=False is passed, and every method takes the level explicitly.

    No monomial table is kept: the fused entries read XPow2NTT / XInvPow2NTT off the twiddle tables, and the naive paths
    materialise the few they need (XPow2NTT above).

    Input ciphertexts are CONSUMED: Pack, Repack[Naive] and Extract[Naive] overwrite their inputs with intermediates, as the
    reference does."""

    def __init__(self, Evaluators: dict, RingSwitchingKeys: dict | None = None, RepackKeys: dict | None = None,
                 ExtractKeys: dict | None = None):
        self.Evaluators = dict(Evaluators)
        self.RingSwitchingKeys = dict(RingSwitchingKeys or {})
        self.RepackKeys, self.ExtractKeys = RepackKeys, ExtractKeys

    def MinLogN(self):
        return min(self.Evaluators)

    def MaxLogN(self):
        return max(self.Evaluators)

    def NewCiphertext(self, logN, level, batch=1):
        r = self.Evaluators[logN].ringQ
        return [Poly(r, level + 1, batch, zero=False) for _ in range(2)]

    @staticmethod
    def _logN(ct):
        return ct[0].N.bit_length() - 1

    def _modulus(self, logN, level):
        Q = 1
        for m in self.Evaluators[logN].ringQ.ModuliChain()[: level + 1]:
            Q *= int(m)
        return Q

    # ---- Split (:173): ctN = ctEvenNHalf(Y) + X ctOddNHalf(Y), Y = X^2; one key switch and one streaming launch
    def Split(self, level, ctN, ctEvenNHalf, ctOddNHalf=None):
        if self.MinLogN() == self.MaxLogN():
            raise ValueError("method is not supported when eval.MinLogN() == eval.MaxLogN()")
        LogN = self._logN(ctN)
        if LogN <= self.MinLogN():
            raise ValueError("ctN.Log() must be greater than eval.MinLogN()")
        if ctEvenNHalf is None:
            raise ValueError("ctEvenNHalf cannot be nil")
        if self._logN(ctEvenNHalf) != LogN - 1:
            raise ValueError("ctEvenNHalf.LogN() must be equal to ctN.LogN()-1")
        if ctOddNHalf is not None and self._logN(ctOddNHalf) != LogN - 1:
            raise ValueError("ctOddNHalf.LogN() must be equal to ctN.LogN()-1")
        o = ctOddNHalf if ctOddNHalf is not None else [None, None]
        check(load().he_ringpack_split(self.Evaluators[LogN].h, level, ctN[0].h, ctN[1].h, self.RingSwitchingKeys[(LogN, LogN - 1)].h,
                                       ctEvenNHalf[0].h, ctEvenNHalf[1].h, o[0].h if o[0] else 0, o[1].h if o[1] else 0))

    def SplitNew(self, level, ctN):
        LogN = self._logN(ctN)
        even, odd = self.NewCiphertext(LogN - 1, level, ctN[0].batch), self.NewCiphertext(LogN - 1, level, ctN[0].batch)
        self.Split(level, ctN, even, odd)
        return even, odd

    # ---- Merge (:376)
    def Merge(self, level, ctEvenNHalf, ctOddNHalf, ctN):
        if self.MinLogN() == self.MaxLogN():
            raise ValueError("method is not supported when eval.MinLogN() == eval.MaxLogN()")
        if ctEvenNHalf is None:
            raise ValueError("ctEvenNHalf cannot be nil")
        if self._logN(ctEvenNHalf) >= self.MaxLogN():
            raise ValueError("ctEvenNHalf.LogN() must be smaller than eval.MaxLogN()")
        LogN = self._logN(ctN)
        if LogN != self._logN(ctEvenNHalf) + 1:
            raise ValueError("ctN.LogN() must be equal to ctEvenNHalf.LogN()+1")
        if ctOddNHalf is not None and self._logN(ctOddNHalf) != LogN - 1:
            raise ValueError("ctEvenNHalf.LogN() and ctOddNHalf.LogN() must be equal")
        o = ctOddNHalf if ctOddNHalf is not None else [None, None]
        check(load().he_ringpack_merge(self.Evaluators[LogN].h, level, ctEvenNHalf[0].h, ctEvenNHalf[1].h, o[0].h if o[0] else 0,
                                       o[1].h if o[1] else 0, self.RingSwitchingKeys[(LogN - 1, LogN)].h, ctN[0].h, ctN[1].h))

    def MergeNew(self, level, ctEvenNHalf, ctOddNHalf):
        if ctEvenNHalf is None:
            raise ValueError("ctEvenNHalf cannot be nil")
        ctN = self.NewCiphertext(self._logN(ctEvenNHalf) + 1, level, ctEvenNHalf[0].batch)
        self.Merge(level, ctEvenNHalf, ctOddNHalf, ctN)
        return ctN

    # ---- Expand (:448).  The map stays ONE batched handle: entry e <-> index e * 2^logGap.  Per level one batched Automorphism
    # over the live entries and one he_ringpack_expand_step.  Returns ([Poly, Poly] of len(indices) entries, indices).
    def Expand(self, level, ct, logGap: int, isNTT: bool = True):
        logN = self._logN(ct)
        if logN not in self.Evaluators:
            raise ValueError(f"eval.Parameters[{logN}] is nil")
        if self.ExtractKeys is None:
            raise ValueError("eval.ExtractKeys is nil")
        if logN not in self.ExtractKeys:
            raise ValueError(f"eval.ExtractKeys[{logN}] is nil")
        ev, gks = self.Evaluators[logN], self.ExtractKeys[logN]
        if getattr(ev.ringQ, "conjugate_invariant", False):
            raise ValueError("method is only supported for ring.Type = ring.Standard")
        rQ = ev.ringQ.AtLevel(level)
        N, gap = 1 << logN, 1 << logGap
        NInv = pow(N, -1, self._modulus(logN, level))
        cur = self.NewCiphertext(logN, level)
        for a, b in zip(ct, cur):
            if not isNTT:
                rQ.NTT(a, b)
                rQ.MulScalarBigint(b, NInv, b)
            else:
                rQ.MulScalarBigint(a, NInv, b)
        m = 1
        L = load()
        for i in range(logN):
            n = 1 << i
            galEl = N // n + 1
            tmp = self.NewCiphertext(logN, level, m)
            ev.Automorphism(level, cur, galEl, gks.GetGaloisKey(galEl), tmp)
            if n >= gap:  # (j + n / gap > 0 for every live j)
                out = self.NewCiphertext(logN, level, 2 * m)
                check(L.he_ringpack_expand_step(ev.ringQ.h, level, i, 0, cur[0].h, cur[1].h, tmp[0].h, tmp[1].h, out[0].h, out[1].h))
                cur, m = out, 2 * m
            else:         # (the lone entry 0: the sum alone, in place)
                check(L.he_ringpack_expand_step(ev.ringQ.h, level, i, 1, cur[0].h, cur[1].h, tmp[0].h, tmp[1].h, cur[0].h, cur[1].h))
        if not isNTT:
            for c in cur:
                rQ.INTT(c, c)
        return cur, [e * gap for e in range(m)]

    # ---- Pack (:573); cts: {index: [Poly, Poly]}, consumed
    def Pack(self, level, cts: dict, inputLogGap: int, zeroGarbageSlots: bool, isNTT: bool = True):
        if len(cts) == 0:
            raise ValueError("len(cts) = 0")
        cts = dict(cts)
        keys = sorted(cts)
        logN = self._logN(cts[keys[0]])
        if logN not in self.Evaluators:
            raise ValueError(f"eval.Parameters[{logN}] is nil")
        if self.RepackKeys is None:
            raise ValueError("eval.RepackKeys is nil")
        if logN not in self.RepackKeys:
            raise ValueError(f"eval.RepackKeys[{logN}] is nil")
        ev, gks = self.Evaluators[logN], self.RepackKeys[logN]
        if getattr(ev.ringQ, "conjugate_invariant", False):
            raise ValueError("procedure is only supported for ring.Type = ring.Standard")
        N = 1 << logN
        if len(keys) > 1:
            gap, logGap = getMinimumGap(keys)
        else:
            gap, logGap = N, logN
        rQ = ev.ringQ.AtLevel(level)
        logStart, logEnd = logN - inputLogGap, logN
        if not zeroGarbageSlots and gap > 0:
            logEnd -= logGap
        if logStart >= logEnd:
            raise ValueError("gaps between ciphertexts is smaller than inputLogGap > N")
        NInv = pow(1 << (logEnd - logStart), -1, self._modulus(logN, level))
        for key in keys:
            for c in cts[key]:
                if not isNTT:
                    rQ.NTT(c, c)
                rQ.MulScalarBigint(c, NInv, c)
        L = load()
        for i in range(logStart, logEnd):
            t = 1 << (logN - 1 - i)
            pairs = []
            for jx in sorted({j & (t - 1) for j in cts if j < 2 * t}):
                a, b = cts.get(jx), cts.get(jx + t)
                if a is not None or b is not None:
                    pairs.append((jx, a, b))
            if not pairs:
                continue
            count = len(pairs)
            nil = [None, None]
            a0, a1 = _harr([(a or nil)[0] for _, a, _ in pairs]), _harr([(a or nil)[1] for _, a, _ in pairs])
            b0, b1 = _harr([(b or nil)[0] for _, _, b in pairs]), _harr([(b or nil)[1] for _, _, b in pairs])
            T = self.NewCiphertext(logN, level, count)
            galEl = 2 * N - 1 if i == 0 else GaloisElement(2 * N, 1 << (i - 1))
            check(L.he_ringpack_pack_pre(ev.ringQ.h, level, logN - 1 - i, count, a0, a1, b0, b1, T[0].h, T[1].h))
            ev.Automorphism(level, T, galEl, gks.GetGaloisKey(galEl), T)
            check(L.he_ringpack_pack_post(ev.ringQ.h, level, count, a0, a1, b0, b1, T[0].h, T[1].h))
            for jx, a, b in pairs:
                if b is not None:
                    if a is None:
                        cts[jx] = b
                    del cts[jx + t]
        out = cts[0]
        if not isNTT:
            for c in out:
                rQ.INTT(c, c)
        return out

    # ---- Extract / ExtractNaive (:52-171): {index: [Poly, Poly] of degree 2^MinLogN}
    def Extract(self, level, ct, idx):
        return self._extract(level, ct, idx, False)

    def ExtractNaive(self, level, ct, idx):
        return self._extract(level, ct, idx, True)

    def _extract(self, level, ct, idx, naive: bool):
        logNMax, logNMin = self._logN(ct), self.MinLogN()
        logNFactor = logNMax - logNMin
        NFactor = 1 << logNFactor
        keys = sorted(idx)
        _, logGap = getMinimumGap(keys)
        tmpCts = {0: ct}
        for i in range(logNFactor):
            t = 1 << i
            logGap = max(0, logGap - 1)
            for j in range(t):
                if j in tmpCts:
                    tmpCts[j], tmpCts[j + t] = self.SplitNew(level, tmpCts[j])
        buckets = {}
        for i in keys:
            buckets.setdefault(i & (NFactor - 1), []).append(i // NFactor)
        rQ = self.Evaluators[logNMin].ringQ
        rL = rQ.AtLevel(level)
        cts = {}
        xinv = {}
        for i, js in buckets.items():
            if naive:
                for j in js:
                    c = self.NewCiphertext(logNMin, level)
                    for a, b in zip(tmpCts[i], c):
                        b.CopyLvl(level, a)
                    for bit in range(logNMin):
                        if (j >> bit) & 1:
                            if bit not in xinv:
                                xinv[bit] = Poly(rQ, level + 1, 1, zero=False)
                                XPow2NTT(rQ, level, bit, True, xinv[bit])
                            for p in c:
                                rL.MulCoeffsMontgomery(p, xinv[bit], p)
                    cts[i + j * NFactor] = c
            else:
                stack, indices = self.Expand(level, tmpCts[i], logGap)
                pos = {j: e for e, j in enumerate(indices)}
                for j in js:
                    if j not in pos:
                        raise ValueError(f"invalid ciphertexts map: index {j} is nil")
                    c = self.NewCiphertext(logNMin, level)
                    for a, b in zip(stack, c):
                        b.CopyBatch(level, 0, a, pos[j], 1)
                    cts[i + j * NFactor] = c
        return cts

    # ---- Repack / RepackNaive (:242-374); cts: {index: [Poly, Poly]}, consumed
    def Repack(self, level, cts: dict):
        return self._repack(level, cts, False)

    def RepackNaive(self, level, cts: dict):
        return self._repack(level, cts, True)

    def _repack(self, level, cts: dict, naive: bool):
        keys = sorted(cts)
        logNMin, logNMax = self._logN(cts[keys[0]]), self.MaxLogN()
        logNFactor = logNMax - logNMin
        NFactor = 1 << logNFactor
        ctsSmallN = [dict() for _ in range(NFactor)]
        for i in keys:
            ctsSmallN[i & (NFactor - 1)][i // NFactor] = cts[i]
        ctsLargeN = {}
        rQ = self.Evaluators[logNMin].ringQ
        rL = rQ.AtLevel(level)
        xpow = {}
        for i in range(NFactor):
            if naive:
                tmpCts = ctsSmallN[i]
                for l in range(logNMin):
                    t = 1 << (logNMin - 1 - l)
                    k = logNMin - 1 - l
                    for jx in sorted({j & (t - 1) for j in tmpCts if t <= j < 2 * t}):
                        a, b = tmpCts.get(jx), tmpCts[jx + t]
                        if k not in xpow:
                            xpow[k] = Poly(rQ, level + 1, 1, zero=False)
                            XPow2NTT(rQ, level, k, False, xpow[k])
                        for p in b:
                            rL.MulCoeffsMontgomery(p, xpow[k], p)
                        if a is not None:
                            for p, r in zip(a, b):
                                rL.Add(p, r, p)
                        else:
                            tmpCts[jx] = b
                        del tmpCts[jx + t]
                if 0 in tmpCts:
                    ctsLargeN[i] = tmpCts[0]
            elif len(ctsSmallN[i]) != 0:
                ctsLargeN[i] = self.Pack(level, ctsSmallN[i], logNMin, True)
        for i in range(logNFactor - 1, -1, -1):
            t = 1 << i
            for j in range(t):
                if ctsLargeN.get(j) is not None or ctsLargeN.get(j + 1) is not None:
                    ctsLargeN[j] = self.MergeNew(level, ctsLargeN.get(j), ctsLargeN.get(j + t))
                    ctsLargeN.pop(j + t, None)
        return ctsLargeN.get(0)


class InnerSumEvaluator:
    """The inner_sum.go methods of rlwe.Evaluator, bound to an Evaluator and a Galois key set."""

    def __init__(self, evaluator: Evaluator, gks: GaloisKeySet):
        self.eval, self.gks = evaluator, gks
        self.ringQ, self.ringP = evaluator.ringQ, evaluator.ringP
        self.be = BasisExtender(self.ringQ, self.ringP)
        self.nth_root = self.ringQ.NthRoot()
        self.logN = self.ringQ.N.bit_length() - 1

    def GaloisElement(self, k: int) -> int:
        return GaloisElement(self.nth_root, k)

    # Evaluator.Trace (core/rlwe/inner_sum.go:36); ct = [c0, c1] at `level`
    def Trace(self, level, ctIn, logN: int, opOut, isNTT: bool = True):
        rQ = self.ringQ.AtLevel(level)
        gap = 1 << (self.logN - logN - 1)
        if logN == 0:
            gap <<= 1
        if gap <= 1:
            if ctIn is not opOut:
                for a, b in zip(opOut, ctIn):
                    a.CopyLvl(level, b)
            return
        ci = getattr(self.ringQ, "conjugate_invariant", False)
        if ci:
            gap >>= 1  # the last step, phi(5^-1), is skipped on Z[X + X^-1] (core/rlwe/inner_sum.go:60-62)
        Q = 1
        for m in self.ringQ.ModuliChain()[: level + 1]:
            Q *= int(m)
        ninv = pow(gap, -1, Q)
        for a, b in zip(ctIn, opOut):
            rQ.MulScalarBigint(a, ninv, b)  # pre-multiplication by (N/n)^-1 (:68-70)
            if not isNTT:
                rQ.NTT(b, b)
        buff = [Poly(self.ringQ, level + 1, opOut[0].batch, zero=False) for _ in range(2)]
        steps = [self.GaloisElement(1 << i) for i in range(logN, self.logN - 1)]
        if logN == 0 and not ci:
            steps.append(self.nth_root - 1)  # X -> X^-1, standard ring only (:97-105)
        for galEl in steps:
            self.eval.Automorphism(level, opOut, galEl, self.gks.GetGaloisKey(galEl), buff)
            for a, b in zip(opOut, buff):
                rQ.Add(a, b, a)
        if not isNTT:
            for b in opOut:
                rQ.INTT(b, b)

    # Evaluator.PartialTracesSum (core/rlwe/inner_sum.go:147)
    def PartialTracesSum(self, level, ctIn, offset: int, n: int, opOut, isNTT: bool = True):
        if n == 0 or offset == 0:
            raise ValueError("partialtrace: invalid parameter (n = 0 or batchSize = 0)")
        levelQ, levelP = level, self.ringP.MaxLevel()
        rQ, rP = self.ringQ.AtLevel(levelQ), self.ringP.AtLevel(levelP)
        B = ctIn[0].batch
        ctInNTT = [Poly(self.ringQ, levelQ + 1, B, zero=False) for _ in range(2)]
        for a, b in zip(ctIn, ctInNTT):
            if not isNTT:
                rQ.NTT(a, b)
            else:
                b.CopyLvl(levelQ, a)
        if n == 1:
            if ctIn is not opOut:
                for a, b in zip(ctIn, opOut):
                    b.CopyLvl(levelQ, a)
        else:
            newQP = lambda: (Poly(self.ringQ, levelQ + 1, B), Poly(self.ringP, levelP + 1, B))
            accQP, cQP = [newQP(), newQP()], [newQP(), newQP()]
            cQ = [cQP[0][0], cQP[1][0]]
            decomp = Decomposition(self.eval, B)
            state, copy = False, True
            i, j = 0, n
            while j > 0:  # binary reading of n (:216)
                self.eval.DecomposeNTT(levelQ, levelP, levelP + 1, ctInNTT[1], True, decomp)
                if j & 1:
                    k = (n - (n & ((2 << i) - 1))) * offset
                    if k != 0:
                        rot = self.GaloisElement(k)
                        gk = self.gks.GetGaloisKey(rot)
                        if copy:
                            self.eval.AutomorphismHoistedLazy(levelQ, ctInNTT, decomp, rot, gk, accQP)
                            copy = False
                        else:
                            self.eval.AutomorphismHoistedLazy(levelQ, ctInNTT, decomp, rot, gk, cQP)
                            for a, c in zip(accQP, cQP):
                                rQ.Add(a[0], c[0], a[0])
                                rP.Add(a[1], c[1], a[1])
                    else:
                        state = True
                        if n & (n - 1):
                            for a, o, c in zip(accQP, opOut, ctInNTT):
                                self.eval.ModDownQPtoQNTT(levelQ, levelP, a[0], a[1], o)
                                rQ.Add(o, c, o)
                        else:
                            for o, c in zip(opOut, ctInNTT):
                                o.CopyLvl(levelQ, c)
                if not state:
                    rot = self.GaloisElement((1 << i) * offset)
                    self.eval.AutomorphismHoisted(levelQ, ctInNTT, decomp, rot, self.gks.GetGaloisKey(rot), cQ)
                    for c, t in zip(ctInNTT, cQ):
                        rQ.Add(c, t, c)
                i, j = i + 1, j >> 1
        if not isNTT:
            for o in opOut:
                rQ.INTT(o, o)

    # InnerSum / Replicate (core/rlwe/inner_sum.go:475 and the scheme-level InnerSum wrappers)
    def InnerSum(self, level, ctIn, batchSize: int, n: int, opOut, isNTT: bool = True):
        self.PartialTracesSum(level, ctIn, batchSize, n, opOut, isNTT)

    def Replicate(self, level, ctIn, batchSize: int, n: int, opOut, isNTT: bool = True):
        self.PartialTracesSum(level, ctIn, -batchSize, n, opOut, isNTT)


def GaloisElementsForInnerSum(nth_root: int, batch: int, n: int):
    """core/rlwe/inner_sum.go:442"""
    rots = set()
    i = 1
    while i < n:
        rots.add(i * batch)
        rots.add((n - (n & ((i << 1) - 1))) * batch)
        i <<= 1
    return sorted({GaloisElement(nth_root, k) for k in rots})


def GaloisElementsForTrace(nth_root: int, logN_ring: int, logN: int):
    """core/rlwe/inner_sum.go:120 (standard ring)"""
    g = [GaloisElement(nth_root, 1 << i) for i in range(logN, logN_ring - 1)]
    if logN == 0:
        g.append(nth_root - 1)
    return g


class CKKSRotations:
    """schemes/ckks Evaluator.Rotate / Conjugate / RotateHoisted / RotateHoistedLazyNew / InnerSum
    (schemes/ckks/evaluator.go:1197-1262, 1283-1300), bound to an Evaluator and a Galois key set."""

    def __init__(self, evaluator: Evaluator, gks: GaloisKeySet):
        self.eval, self.gks = evaluator, gks
        self.ise = InnerSumEvaluator(evaluator, gks)
        self.nth_root = evaluator.ringQ.NthRoot()

    def Rotate(self, level, op0, k: int, opOut):
        g = GaloisElement(self.nth_root, k)
        self.eval.Automorphism(level, op0, g, self.gks.GetGaloisKey(g), opOut)

    def Conjugate(self, level, op0, opOut):
        g = self.nth_root - 1  # GaloisElementOrderTwoOrthogonalSubgroup (core/rlwe/params.go:592)
        self.eval.Automorphism(level, op0, g, self.gks.GetGaloisKey(g), opOut)

    def RotateHoisted(self, level, ctIn, rotations, opOut: dict):
        levelP = self.eval.ringP.MaxLevel()
        decomp = Decomposition(self.eval, ctIn[0].batch)
        self.eval.DecomposeNTT(level, levelP, levelP + 1, ctIn[1], True, decomp)
        for i in rotations:
            g = GaloisElement(self.nth_root, i)
            self.eval.AutomorphismHoisted(level, ctIn, decomp, g, self.gks.GetGaloisKey(g), opOut[i])

    def RotateHoistedLazyNew(self, level, rotations, ct, decomp: Decomposition) -> dict:
        levelP, B, out = self.eval.ringP.MaxLevel(), ct[0].batch, {}
        for i in rotations:
            if i != 0:
                out[i] = [(Poly(self.eval.ringQ, level + 1, B, zero=False), Poly(self.eval.ringP, levelP + 1, B, zero=False)) for _ in range(2)]
                g = GaloisElement(self.nth_root, i)
                self.eval.AutomorphismHoistedLazy(level, ct, decomp, g, self.gks.GetGaloisKey(g), out[i])
        return out

    def InnerSum(self, level, ctIn, batchSize: int, n: int, opOut, slots: int | None = None):
        N = slots if slots is not None else self.eval.ringQ.N // 2
        l = n * batchSize
        if n <= 0 or batchSize <= 0:
            raise ValueError("innersum: invalid parameter (n <= 0 or batchSize <= 0)")
        if l > N:
            raise ValueError(f"innersum: invalid parameters (n*batchSize={l} > #slots={N})")
        if l & (l - 1):
            raise ValueError(f"innersum: invalid parameters (n*batchSize={l} does not divide #slots={N})")
        self.ise.PartialTracesSum(level, ctIn, batchSize, n, opOut)


def ConcurrentCalls(op: str, callers, level: int, iters: int, t: int = 0, sync_each: bool = False) -> float:
    """The reference's parallel benchmark shape (b.RunParallel, schemes/ckks/ckks_benchmarks_test.go:116-207) on OS threads inside
    the library (he_debug_concurrent_mul_relin, include/hering_debug.h).  op "ckks_mulrelin" / "bgv_mulrelin" (t = plaintext
    modulus): callers = [(ctx, evaluator, op0, op1, rlk, opOut), ...]; "rotate" (t = Galois element): [(ctx, evaluator, ct, None,
    galois key, ctOut)]; "relinearize": [(ctx, evaluator, ct3, None, rlk, ctOut)]; "gadget_product": [(ctx, evaluator, [cx], None,
    key, ctOut)] -- all with batch-1 polynomials.  Caller i makes `iters` calls on its own handles, synchronising its context
    after every call (sync_each) or once at the end.  Returns the wall time in seconds."""
    code = {"ckks_mulrelin": 0, "bgv_mulrelin": 1, "rotate": 2, "relinearize": 3, "gadget_product": 4}[op]
    n = len(callers)
    arr = lambda f: (H * n)(*[f(c) for c in callers])
    pick = lambda c, which, i: (c[which][i].h if c[which] is not None and len(c[which]) > i else c[2][0].h)
    wall = C.c_double()
    check(load().he_debug_concurrent_mul_relin(
        n, iters, int(sync_each), code, level, t, arr(lambda c: c[0].h), arr(lambda c: c[1].h), arr(lambda c: pick(c, 2, 0)),
        arr(lambda c: pick(c, 2, 1)), arr(lambda c: pick(c, 3, 0) if code < 2 else pick(c, 2, 2)), arr(lambda c: pick(c, 3, 1)),
        arr(lambda c: c[4].h), arr(lambda c: c[5][0].h), arr(lambda c: c[5][1].h), C.byref(wall)))
    return float(wall.value)


def ConcurrentMulRelin(callers, level: int, iters: int, t: int = 0, sync_each: bool = False) -> float:
    """ConcurrentCalls for BGVMulRelin (t != 0) / CKKSMulRelin"""
    return ConcurrentCalls("bgv_mulrelin" if t != 0 else "ckks_mulrelin", callers, level, iters, t, sync_each)


# ----------------------------------------------------------------------------------------------------
# rlwe.Scale, rlwe.MetaData, rlwe.Ciphertext and rlwe.Plaintext (core/rlwe/scale.go, metadata.go, ciphertext.go, plaintext.go): what
# ckks.Evaluator (lattigo_amd.ckks) keeps beside the device polynomials of an element.
# ----------------------------------------------------------------------------------------------------
ScalePrecision = 128  # core/rlwe/scale.go:17


class Scale:
    """rlwe.Scale: a big.Float of 128 bits.  Mul / Div round the exact result to 128 bits, nearest even; Int truncates; Float64
    rounds to nearest even.  The value is held as the exact rational of that float (Value)."""

    __slots__ = ("Value",)

    def __init__(self, s=1):
        from fractions import Fraction
        from .polyeval import _round_bits
        v = s.Value if isinstance(s, Scale) else Fraction(s)  # an int or a float64 is taken exactly, then rounded (NewScale, scale.go:29-56)
        if v < 0:
            raise ValueError("a scale cannot be negative")
        self.Value = _round_bits(v, ScalePrecision)

    def Mul(self, s1) -> "Scale":
        return Scale(self.Value * Scale(s1).Value)

    def Div(self, s1) -> "Scale":
        return Scale(self.Value / Scale(s1).Value)

    def Cmp(self, s1) -> int:
        o = Scale(s1).Value
        return (self.Value > o) - (self.Value < o)

    def Equal(self, s1) -> bool:
        return self.Cmp(s1) == 0

    def Max(self, s1) -> "Scale":
        return Scale(self) if self.Cmp(s1) >= 0 else Scale(s1)

    def Min(self, s1) -> "Scale":
        return Scale(self) if self.Cmp(s1) <= 0 else Scale(s1)

    def Int(self) -> int:
        return self.Value.numerator // self.Value.denominator

    BigInt = Int

    def Uint64(self) -> int:
        return min(self.Int(), 0xFFFFFFFFFFFFFFFF)  # big.Float.Uint64 saturates

    def Float64(self) -> float:
        return self.Value.numerator / self.Value.denominator  # int / int is correctly rounded, ties to even

    def __repr__(self):
        return f"Scale({self.Float64()!r})"


def NewScale(s) -> Scale:
    return Scale(s)


class MetaData:
    """rlwe.MetaData (metadata.go): PlaintextMetaData (Scale, LogDimensions, IsBatched) and CiphertextMetaData (IsNTT, IsMontgomery)"""

    __slots__ = ("Scale", "IsNTT", "IsMontgomery", "IsBatched", "LogDimensions")

    def __init__(self, Scale_=1, IsNTT=True, IsMontgomery=False, IsBatched=True, LogDimensions=(0, 0)):
        self.Scale, self.IsNTT, self.IsMontgomery, self.IsBatched = Scale(Scale_), IsNTT, IsMontgomery, IsBatched
        self.LogDimensions = tuple(LogDimensions)  # (Rows, Cols)

    def copy(self) -> "MetaData":
        return MetaData(self.Scale, self.IsNTT, self.IsMontgomery, self.IsBatched, self.LogDimensions)


class Element:
    """rlwe.Element[ring.Poly] over device polynomials: Value[i] is a Poly of `batch` entries; the level of the element is kept
    beside them (a Poly keeps its allocated height: Resize to a lower level drops no memory, as the reference's Resize keeps the
    backing arrays)."""

    def __init__(self, ringQ: Ring, degree: int, level: int, batch: int = 1, Value=None, MetaData_: MetaData | None = None):
        self.ringQ, self.batch, self.level = ringQ, batch, level
        self.Value = list(Value) if Value is not None else [Poly(ringQ, level + 1, batch) for _ in range(degree + 1)]
        self.MetaData = MetaData_ if MetaData_ is not None else MetaData()

    Scale = property(lambda self: self.MetaData.Scale, lambda self, s: setattr(self.MetaData, "Scale", Scale(s)))
    IsNTT = property(lambda self: self.MetaData.IsNTT, lambda self, v: setattr(self.MetaData, "IsNTT", v))
    IsBatched = property(lambda self: self.MetaData.IsBatched, lambda self, v: setattr(self.MetaData, "IsBatched", v))
    LogDimensions = property(lambda self: self.MetaData.LogDimensions, lambda self, v: setattr(self.MetaData, "LogDimensions", tuple(v)))

    def El(self):
        return self

    def Degree(self) -> int:
        return len(self.Value) - 1

    def Level(self) -> int:
        return self.level

    def Resize(self, degree: int, level: int):
        """Element.Resize (element.go:147-176): components are dropped or added (zero), the level is lowered or raised (a raised
        level needs the height: a component that is too short is replaced by a zero-extended copy)"""
        self.Value = self.Value[: degree + 1]
        for i, p in enumerate(self.Value):
            if p.n_limbs < level + 1:
                q = Poly(self.ringQ, level + 1, self.batch)
                q.CopyLvl(p.n_limbs - 1, p)
                self.Value[i] = q
        while len(self.Value) < degree + 1:
            self.Value.append(Poly(self.ringQ, level + 1, self.batch))
        self.level = level

    def CopyNew(self):
        out = object.__new__(type(self))
        Element.__init__(out, self.ringQ, self.Degree(), self.level, self.batch, MetaData_=self.MetaData.copy())
        for a, b in zip(out.Value, self.Value):
            a.CopyLvl(self.level, b)
        return out


class Ciphertext(Element):
    """rlwe.Ciphertext"""


class Plaintext(Element):
    """rlwe.Plaintext: an element of degree 0"""

    def __init__(self, ringQ: Ring, level: int, batch: int = 1, Value=None, MetaData_: MetaData | None = None):
        super().__init__(ringQ, 0, level, batch, Value=Value, MetaData_=MetaData_)
