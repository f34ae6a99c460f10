"""circuits/common/lintrans on the device (include/hering_lintrans.h): plaintext-matrix x ciphertext products by diagonals.
``LinearTransformation`` holds the encoded diagonals as QP polynomials (NTT + Montgomery) and the library's plan of their
evaluation; ``Evaluator.EvaluateMany`` is ONE native call (he_lintrans_evaluate_many): the decomposition, the hoisted
pre-rotations, the grouped multiply-accumulate kernel, the giant steps and the ModDowns are composed inside the library.
``Encode`` (lintrans.go:205-292) works with both ``ckks.Encoder`` and ``bgv.Encoder`` through their ``EncodeQP``."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from lattigo_amd._lib import H, check, load
from lattigo_amd.ring import Poly
from lattigo_amd import blindrot, rlwe


def _ints(v):
    v = [int(x) for x in v]
    return (C.c_int * max(len(v), 1))(*v), len(v)


def BSGSIndex(nonZeroDiags, slots: int, N1: int):
    """lintrans.go:344: ({giant step: sorted baby steps}, sorted giant steps, sorted baby steps)"""
    d, n = _ints(nonZeroDiags)
    cap = max(min(n, slots), 1)
    r1, r2, idx = (C.c_int * cap)(), (C.c_int * cap)(), (C.c_int * max(2 * n, 1))()
    n1, n2 = C.c_int(), C.c_int()
    check(load().he_lintrans_bsgs_index(d, n, slots, N1, r1, C.byref(n1), r2, C.byref(n2), idx))
    index: dict = {}
    for k in range(n):
        index.setdefault(int(idx[2 * k]), []).append(int(idx[2 * k + 1]))
    for j in index:
        index[j].sort()
    return index, [int(r1[i]) for i in range(n1.value)], [int(r2[i]) for i in range(n2.value)]


def FindBestBSGSRatio(nonZeroDiags, maxN: int, logMaxRatio: int) -> int:
    """lintrans.go:321"""
    d, n = _ints(nonZeroDiags)
    out = C.c_int()
    check(load().he_lintrans_find_best_bsgs_ratio(d, n, maxN, logMaxRatio, C.byref(out)))
    return out.value


def GaloisElements(evaluator: rlwe.Evaluator, diags, slots: int, logBSGSRatio: int):
    """lintrans.go:297 on the evaluator's ring"""
    d, n = _ints(diags)
    cap = 2 * n + 2
    out, got = (C.c_uint64 * cap)(), C.c_size_t()
    check(load().he_lintrans_galois_elements(evaluator.h, d, n, slots, logBSGSRatio, out, cap, C.byref(got)))
    return [int(out[i]) for i in range(got.value)]


@dataclass
class Parameters:
    """lintrans.Parameters (lintrans.go:20-62)"""
    DiagonalsIndexList: list
    LevelQ: int
    LevelP: int
    Scale: float
    LogDimensions: tuple  # (Rows, Cols)
    LogBabyStepGiantStepRatio: int = 0


class LinearTransformation:
    """lintrans.LinearTransformation (lintrans.go:127): Vec[k] = (Q, P) device polynomials of the k-th non-zero diagonal.  The
    native handle (he_lintrans_create) is made on first use, once every diagonal is in place, and again after a change of Vec."""

    def __init__(self, evaluator: rlwe.Evaluator, Vec: dict, LevelQ: int, LevelP: int, LogDimensions, N1: int = 0, Scale=1.0,
                 LogBabyStepGiantStepRatio: int = 0):
        self.eval, self.Vec, self.LevelQ, self.LevelP, self.N1 = evaluator, Vec, LevelQ, LevelP, N1
        self.LogDimensions, self.Scale, self.LogBabyStepGiantStepRatio = tuple(LogDimensions), Scale, LogBabyStepGiantStepRatio
        self.slots = 1 << self.LogDimensions[1]
        self._h, self._made_for, self._group = None, None, 0

    def GaloisElements(self):
        return GaloisElements(self.eval, list(self.Vec.keys()), self.slots, self.LogBabyStepGiantStepRatio)

    def BSGSIndex(self):
        return BSGSIndex(list(self.Vec.keys()), self.slots, self.N1)

    def SetGroup(self, G: int):
        """giant steps per launch of the grouped kernel: 0 (the library's default), 1, 2 or 4"""
        self._group = int(G)
        if self._h:
            check(load().he_lintrans_set_group(self._h, self._group))

    @property
    def h(self):
        key = tuple((k, q.h, p.h) for k, (q, p) in self.Vec.items())
        if self._h is None or key != self._made_for:
            self._release()
            n = len(self.Vec)
            d, _ = _ints(self.Vec.keys())
            hq, hp = (H * n)(*[q.h for q, _ in self.Vec.values()]), (H * n)(*[p.h for _, p in self.Vec.values()])
            h = H()
            check(load().he_lintrans_create(self.eval.h, self.LevelQ, self.LevelP, self.LogDimensions[1], self.N1, n, d, hq, hp, C.byref(h)))
            self._h, self._made_for = h.value, key
            if self._group:
                check(load().he_lintrans_set_group(self._h, self._group))
        return self._h

    def _release(self):
        if self._h:
            load().he_lintrans_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass


def NewLinearTransformation(evaluator: rlwe.Evaluator, ltparams: Parameters) -> LinearTransformation:
    """lintrans.go:148: zero diagonals at (LevelQ, LevelP) for the indices of ltparams"""
    cols = 1 << ltparams.LogDimensions[1]
    ringQ, ringP = evaluator.ringQ, evaluator.ringP
    new = lambda: (Poly(ringQ, ltparams.LevelQ + 1), Poly(ringP, ltparams.LevelP + 1))
    vec = {}
    if ltparams.LogBabyStepGiantStepRatio < 0:
        N1 = 0
        for i in ltparams.DiagonalsIndexList:
            vec[i + cols if i < 0 else i] = new()
    else:
        N1 = FindBestBSGSRatio(ltparams.DiagonalsIndexList, cols, ltparams.LogBabyStepGiantStepRatio)
        index, _, _ = BSGSIndex(ltparams.DiagonalsIndexList, cols, N1)
        for j in index:
            for i in index[j]:
                vec[j + i] = new()
    return LinearTransformation(evaluator, vec, ltparams.LevelQ, ltparams.LevelP, ltparams.LogDimensions, N1, ltparams.Scale,
                                ltparams.LogBabyStepGiantStepRatio)


def _diag_at(diagonals: dict, i: int, slots: int):
    """Diagonals.At (lintrans.go:96-122): index i, or its representative on the other side of zero"""
    if i in diagonals:
        return diagonals[i]
    j = i - slots if i > 0 else i + slots
    if i == 0 or j not in diagonals:
        raise KeyError(f"cannot At[{i} or {j}]: diagonal does not exist")
    return diagonals[j]


def Encode(encoder, diagonals: dict, lt: LinearTransformation):
    """lintrans.go:205-292: the non-zero diagonals {index: [rows * cols] values} onto the allocated transformation -- in the BSGS
    form each diagonal of giant step j rotated by -j first -- through encoder.EncodeQP (NTT + Montgomery)."""
    rows, cols = 1 << lt.LogDimensions[0], 1 << lt.LogDimensions[1]

    def embed(v, rot, vec):
        v = np.asarray(v).reshape(rows, cols)
        rot &= cols - 1
        if rot:
            v = np.roll(v, -rot, axis=1)  # utils.RotateSliceAllocFree: to the left
        encoder.EncodeQP(v.reshape(-1), vec[0], vec[1], Scale=lt.Scale, levelQ=lt.LevelQ, levelP=lt.LevelP, **_slots_kw(encoder, lt))

    if lt.N1 == 0:
        for i in diagonals:
            idx = i + cols if i < 0 else i
            if idx not in lt.Vec:
                raise KeyError(f"cannot Encode: plaintext diagonal [{idx}] does not exist")
            embed(_diag_at(diagonals, i, cols), 0, lt.Vec[idx])
    else:
        index, _, _ = lt.BSGSIndex()
        for j in index:
            for i in index[j]:
                if i + j not in lt.Vec:
                    raise KeyError("cannot Encode: input does not match the same non-zero diagonals")
                embed(_diag_at(diagonals, i + j, cols), -j & (cols - 1), lt.Vec[i + j])
    return lt  # (the words changed, the polynomials did not: a handle made earlier reads them at evaluation and stays good)


def _slots_kw(encoder, lt):
    # ckks.Encoder.EncodeQP takes the slot count of the values; bgv.Encoder's has no such argument: it always fills the ring
    import inspect
    takes = "LogSlots" in inspect.signature(encoder.EncodeQP).parameters
    return {"LogSlots": lt.LogDimensions[0] + lt.LogDimensions[1]} if takes else {}


class Evaluator:
    """lintrans.Evaluator (lintrans_evaluator.go:12) over an rlwe.Evaluator and its Galois keys {galEl: EvaluationKey}."""

    def __init__(self, evaluator: rlwe.Evaluator, galois_keys):
        self.eval = evaluator
        keys = galois_keys.keys if isinstance(galois_keys, rlwe.GaloisKeySet) else galois_keys
        if isinstance(galois_keys, blindrot.GaloisKeySet):
            self.gks = galois_keys
        else:  # (no key at all: only transformations of the zero diagonal alone can be evaluated)
            self.gks = blindrot.GaloisKeySet(evaluator, dict(keys)) if len(keys) else None
        self._set = self.gks.h if self.gks is not None else 0

    def EvaluateMany(self, ctLevel: int, ctIn, linearTransformations, opOut):
        """:27: ctIn = [c0, c1] (NTT) at ctLevel; opOut = one [c0, c1] per transformation"""
        if len(opOut) < len(linearTransformations):
            raise ValueError("output *rlwe.Ciphertext slice is too small")
        n = len(linearTransformations)
        lts = (H * n)(*[lt.h for lt in linearTransformations])
        o0, o1 = (H * n)(*[o[0].h for o in opOut[:n]]), (H * n)(*[o[1].h for o in opOut[:n]])
        check(load().he_lintrans_evaluate_many(self.eval.h, self._set, ctLevel, ctIn[0].h, ctIn[1].h, n, lts, o0, o1))

    def Evaluate(self, ctLevel: int, ctIn, linearTransformation, opOut):
        """:122"""
        check(load().he_lintrans_evaluate(self.eval.h, self._set, ctLevel, ctIn[0].h, ctIn[1].h, linearTransformation.h, opOut[0].h, opOut[1].h))

    def EvaluateNew(self, ctLevel: int, ctIn, linearTransformation):
        """:109: the result at min(ctLevel, LevelQ)"""
        level = min(ctLevel, linearTransformation.LevelQ)
        B = ctIn[0].batch
        out = [Poly(self.eval.ringQ, level + 1, B, zero=False), Poly(self.eval.ringQ, level + 1, B, zero=False)]
        self.Evaluate(ctLevel, ctIn, linearTransformation, out)
        return out

    def EvaluateSequential(self, ctLevel: int, ctIn, linearTransformations, opOut, rescale=None):
        """:128: the transformations one after the other, each on the result of the one before (`rescale(level, ct)`, when given,
        is applied between two of them and returns the new level); the last one writes opOut."""
        cur, level = ctIn, ctLevel
        for k, lt in enumerate(linearTransformations):
            if k == len(linearTransformations) - 1:
                self.Evaluate(level, cur, lt, opOut)
                return min(level, lt.LevelQ)
            cur = self.EvaluateNew(level, cur, lt)
            level = min(level, lt.LevelQ)
            if rescale is not None:
                level = rescale(level, cur)
        return level
