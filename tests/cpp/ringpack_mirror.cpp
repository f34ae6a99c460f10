#include "hering.hpp"
using namespace hering;
void use(const Evaluator &ev, const Ring &rN, const Ring &rH, const EvaluationKey &k0, const EvaluationKey &k1, Ciphertext &ct) {
    RingPackingEvaluator rp(ev, rH, k0, k1);
    auto eo = rp.SplitNew(ct);
    rp.Split(ct, eo.first, nullptr);
    Ciphertext m = rp.MergeNew(eo.first, &eo.second);
    rp.Merge(eo.first, nullptr, m);
    Poly p = rN.NewPoly(), e = rH.NewPoly(), o = rH.NewPoly();
    XPow2NTT(rN, 0, 0, true, p);
    SplitNTT(rN, 0, p, e, &o);
    MergeNTT(rN, 0, e, &o, p);
    ExpandStep(rN, 0, 0, true, ct, ct, ct);
    std::vector<const Poly *> a0{&ct.Value[0]}, a1{&ct.Value[1]}, b0{nullptr}, b1{nullptr};
    PackPre(rN, 0, 0, a0, a1, b0, b1, m);
    PackPost(rN, 0, a0, a1, b0, b1, m);
}
