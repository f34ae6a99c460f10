"""tests/drivers/polyeval.py with its baby steps handed to the library: the power basis and the giant steps stay the driver's
compositions of the operator entries, every baby step of an evaluation goes through ONE he_polyeval_leaves call (the leaf-group
kernel) on the handle lattigo_amd.polyeval planned.  Used by tests/test_gpu_polyeval.py and tools/polyeval_bench.py."""
from __future__ import annotations

import lattigo_amd as la
from drivers import polyeval as PE
from drivers import schemes as S
from lattigo_amd import polyeval as NP


class NativeLeaves(PE.PolynomialEvaluator):
    """tests/drivers/polyeval.py with EvaluateBabyStep replaced: ALL baby steps of an evaluation in one he_polyeval_leaves call
    on the handle lattigo_amd.polyeval planned; the power basis and the giant steps stay the driver's"""

    def __init__(self, evaluator, ring, G=0):
        super().__init__(evaluator)
        self.ring, self.G = ring, G
        self.scheme = NP.BGVScheme(evaluator.Q, evaluator.t) if self.bgv else NP.CKKSScheme.for_ring(ring)
        self.planned, self._done, self.calls, self._plans = None, None, 0, {}

    def plan(self, pol, level, scale, target, powers=None):
        """planned once per (polynomial, input, target): the handle keeps the words on the device"""
        key = (tuple(pol.Coeffs), pol.Basis, pol.IsEven, pol.IsOdd, pol.Lazy, level, scale, target, None if powers is None else tuple(sorted(powers.items())))
        if key not in self._plans:
            mine = NP.Polynomial(pol.Coeffs, pol.Basis, pol.IsEven, pol.IsOdd, pol.Lazy)
            self._plans[key] = mine.Plan(self.scheme, level, scale, target, powers=powers, ring=self.ring, copy_input=powers is None)
            self._plans[key].SetGroup(self.G)
        self.planned, self._done = self._plans[key], None
        return self.planned

    def Evaluate(self, ct, pol, targetScale):
        self.plan(pol, ct.level, ct.Scale, targetScale)
        return super().Evaluate(ct, pol, targetScale)

    def EvaluateBabyStep(self, poly, pb):
        if self._done is None:
            pl, ev = self.planned, self.eval
            B = pb.Value[1].Value[0].batch
            outs = []
            for f in pl.leaves:
                o = S.Ciphertext([la.Poly(self.ring, f["level"] + 1, B, zero=False) for _ in range(f["ct_degree"] + 1)], f["level"], 1)
                o.Scale = f["out_scale"]
                outs.append(o)
            pl.EvaluatePolynomialFromPowerBasis({k: x.Value for k, x in pb.Value.items()}, [o.Value for o in outs])
            self.calls += 1
            self._done = list(zip(pl.leaves, outs))
        f, o = self._done.pop(0)
        assert (poly.Degree(), poly.Level, poly.Scale) == (f["degree"], f["level"], f["scale"])  # the driver's plan = the mirror's
        return PE._BabyStep(poly.Degree(), o)
