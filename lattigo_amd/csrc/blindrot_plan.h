// The schedule of a blind rotation (core/rgsw/blindrot/evaluator.go:135-280), decided on the host: blindrot_ops() restates
// BlindRotateCore for ONE row `a` as the list of operations the reference applies to that row's accumulator, and
// blindrot_merge() merges the lists of a batch into rounds of one automorphism-select launch and one external-product-select
// launch.  Host only, no HIP or library includes: tests/cpp/blindrot_plan_test.cpp runs it on the CPU.
//
// The reference's behaviour, reproduced word for word:
//  - getGaloisElementInverseMap (:232-255) stores map[g^i] = i and map[2N - g^i] = -i for 0 <= i < N/2, so map[1] = 0 and
//    map[2N - 1] = -0 = 0; a key the map does not hold (0, and every even word) reads as 0 (:270).  a[i] in {0, 1, 2N - 1}
//    therefore all land in set 0, which the LAST line of BlindRotateCore serves (:181): the sign of such an a[i] is lost.
//  - a non-zero even a[i] is no element of Z_2N^*; the reference panics there (:266-268) and blindrot_ops() returns false before
//    anything is listed.
//  - the negative sets are walked for k = -(N/2 - 1) .. -1 (:156-160), then k = 2N is looked up (:163) -- a key no set has, since
//    discrete logs lie in (-N/2, N/2) -- with v = 0 and its result thrown away: the step counts to v = 1, emits nothing, and the
//    caller's v KEEPS the value the negative walk left.  Then Automorphism(acc, 2N - 5) (:169), the positive sets for
//    k = N/2 - 1 .. 1 (:174-178) continuing with that v, and set 0 with v = 0 (:181).
//  - a step (evaluateFromDiscreteLogSets, :189-229): when set k exists, a pending v != 0 is flushed as Automorphism(g^v) and the
//    set's keys are multiplied in, in the order their indices appear in `a`; then v is incremented and flushed when it reaches
//    windowSize = 10 (keys.go:14) or when k == 1.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace blindrot {
constexpr int kWindowSize = 10;       // core/rgsw/blindrot/keys.go:14
constexpr uint64_t kGaloisGen = 5;    // ring.GaloisGen

enum OpKind { OP_AUTOMORPHISM = 0, OP_EXTERNAL_PRODUCT = 1 };
struct Op {
    int kind;      // OP_AUTOMORPHISM: arg is the Galois element; OP_EXTERNAL_PRODUCT: arg is the index of the blind rotation key
    uint64_t arg;
};

// rlwe.Parameters.GaloisElement(k) on a standard ring: GaloisGen^k mod 2N
inline uint64_t galois_element(int logN, int k) {
    const uint64_t mask = ((uint64_t)2 << logN) - 1;
    uint64_t e = (uint64_t)(int64_t)k & mask, g = kGaloisGen, r = 1;
    for (; e; e >>= 1, g = g * g & mask)
        if (e & 1) r = r * g & mask;
    return r;
}
// the Galois elements BlindRotateCore can ask for (keys.go:41-60): g^1 .. g^windowSize and 2N - g
inline std::vector<uint64_t> galois_elements(int logN) {
    std::vector<uint64_t> out;
    for (int v = 1; v <= kWindowSize; v++) out.push_back(galois_element(logN, v));
    out.push_back(((uint64_t)2 << logN) - kGaloisGen);
    return out;
}

// BlindRotateCore for one row: false when some a[i] is a non-zero even word (or lies outside [0, 2N)); `ops` is then untouched
inline bool blindrot_ops(int logN, const uint64_t *a, int n_lwe, std::vector<Op> *ops) {
    if (logN < 2 || logN > 30 || n_lwe < 0 || (n_lwe > 0 && !a)) return false;
    const int64_t N = (int64_t)1 << logN, twoN = N << 1, Nhalf = N >> 1;
    for (int i = 0; i < n_lwe; i++)
        if (a[i] >= (uint64_t)twoN || ((a[i] & 1) != 1 && a[i] != 0)) return false;
    // getGaloisElementInverseMap: dlog[w] (0 where the map has no key)
    std::vector<int32_t> dlog((size_t)twoN, 0);
    uint64_t pow = 1;
    for (int64_t i = 0; i < Nhalf; i++) {
        dlog[pow] = (int32_t)i;
        dlog[(uint64_t)twoN - pow] = (int32_t)-i;
        pow = pow * kGaloisGen & (uint64_t)(twoN - 1);
    }
    // getDiscreteLogSets: sets[k + N/2] = the indices i with dlog[a[i]] == k, in order (k in (-N/2, N/2))
    std::vector<std::vector<int32_t>> sets((size_t)N);
    for (int i = 0; i < n_lwe; i++) sets[(size_t)(dlog[a[i]] + Nhalf)].push_back(i);
    std::vector<Op> out;
    // evaluateFromDiscreteLogSets
    auto step = [&](int64_t k, int v) -> int {
        const bool in_range = k > -Nhalf && k < Nhalf;
        const std::vector<int32_t> *set = in_range && !sets[(size_t)(k + Nhalf)].empty() ? &sets[(size_t)(k + Nhalf)] : nullptr;
        if (set) {
            if (v != 0) {
                out.push_back(Op{OP_AUTOMORPHISM, galois_element(logN, v)});
                v = 0;
            }
            for (int32_t j : *set) out.push_back(Op{OP_EXTERNAL_PRODUCT, (uint64_t)j});
        }
        v++;
        if (v == kWindowSize || k == 1) {
            out.push_back(Op{OP_AUTOMORPHISM, galois_element(logN, v)});
            v = 0;
        }
        return v;
    };
    int v = 0;
    for (int64_t i = Nhalf - 1; i > 0; i--) v = step(-i, v);
    (void)step(twoN, 0);
    out.push_back(Op{OP_AUTOMORPHISM, (uint64_t)twoN - kGaloisGen});
    for (int64_t i = Nhalf - 1; i > 0; i--) v = step(i, v);
    (void)step(0, 0);
    ops->swap(out);
    return true;
}

// One round of the batched route: entry b takes the automorphism with Galois element gal[b] (0: none), then the external product
// with key prod[b] (-1: none).
struct Round {
    std::vector<uint64_t> gal;
    std::vector<int32_t> prod;
};
// how many rounds one list takes on its own
inline size_t blindrot_round_count(const std::vector<Op> &ops) {
    size_t n = 0;
    for (size_t p = 0; p < ops.size(); n++) {
        if (ops[p].kind == OP_AUTOMORPHISM) p++;
        if (p < ops.size() && ops[p].kind == OP_EXTERNAL_PRODUCT) p++;
    }
    return n;
}
// In a round an entry consumes its next operation if that is an automorphism, then its next operation if that is an external
// product: every entry's subsequence of the rounds is its own list in order, and there are as many rounds as the longest entry
// takes on its own.
inline std::vector<Round> blindrot_merge(const std::vector<std::vector<Op>> &lists) {
    const size_t B = lists.size();
    std::vector<size_t> pos(B, 0);
    std::vector<Round> rounds;
    for (;;) {
        bool any = false;
        for (size_t b = 0; b < B; b++) any = any || pos[b] < lists[b].size();
        if (!any) break;
        Round r;
        r.gal.assign(B, 0);
        r.prod.assign(B, -1);
        for (size_t b = 0; b < B; b++) {
            const std::vector<Op> &l = lists[b];
            if (pos[b] < l.size() && l[pos[b]].kind == OP_AUTOMORPHISM) r.gal[b] = l[pos[b]++].arg;
            if (pos[b] < l.size() && l[pos[b]].kind == OP_EXTERNAL_PRODUCT) r.prod[b] = (int32_t)l[pos[b]++].arg;
        }
        rounds.push_back(std::move(r));
    }
    return rounds;
}
}  // namespace blindrot
