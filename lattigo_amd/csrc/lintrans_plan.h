// The index of a linear transformation (circuits/common/lintrans/lintrans.go:297-377) and the launch plan of its evaluation,
// decided on the host.  bsgs_index() restates BSGSIndex, find_best_bsgs_ratio() FindBestBSGSRatio and galois_elements()
// GaloisElements; build_plan() cuts the sorted giant steps of the baby-step giant-step form into groups of at most G members,
// each served by ONE launch of the grouped multiply-accumulate kernel per ring part.  Host only, no HIP or library includes:
// tests/cpp/lintrans_plan_test.cpp runs it on the CPU.
//
// The reference's behaviour, reproduced:
//  - BSGSIndex reduces a rotation with `& (slots - 1)`, files it under the giant step ((rot / N1) * N1) & (slots - 1) with the
//    baby step rot & (N1 - 1), and sorts each giant step's baby steps; rotN1 / rotN2 are the sorted sets of both.
//  - FindBestBSGSRatio walks N1 = 1, 2, 4, ... < maxN and compares float64(nbN2) / float64(nbN1) with float64(1 << logMaxRatio):
//    equal returns N1, greater returns N1 / 2 (0 when N1 is 1); a division by zero gives +Inf, -Inf or NaN as in IEEE 754 and
//    takes part in the two comparisons as such (NaN compares false twice and the walk goes on).
//  - GaloisElements: logBSGSRatio < 0 lists the baby steps of BSGSIndex(diags, slots, slots) -- every rotation, the zero one
//    included --, otherwise the sorted union of the giant and the baby steps at N1 = FindBestBSGSRatio; every rotation k becomes
//    GaloisGen^(k mod NthRoot) mod NthRoot.
// There is no cap on the number of terms: the lists are as long as the transformation needs.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <map>
#include <set>
#include <vector>

namespace lintrans {
constexpr uint64_t kGaloisGen = 5;  // ring.GaloisGen
constexpr int kMaxGroup = 4;        // the largest group the grouped kernel is built for

// rlwe.Parameters.GaloisElement(k): GaloisGen^(k mod NthRoot) mod NthRoot (NthRoot a power of two)
inline uint64_t galois_element(uint64_t nth_root, int64_t k) {
    const uint64_t mask = nth_root - 1;
    uint64_t e = (uint64_t)k & mask, g = kGaloisGen, r = 1;
    for (; e; e >>= 1, g = g * g & mask)
        if (e & 1) r = r * g & mask;
    return r;
}

struct BsgsIndex {
    std::map<int, std::vector<int>> index;  // giant step -> its sorted baby steps
    std::vector<int> rotN1, rotN2;          // sorted
};
// BSGSIndex (lintrans.go:344); slots and N1 are powers of two (N1 >= 1)
inline BsgsIndex bsgs_index(const int *diags, int n, int slots, int N1) {
    BsgsIndex out;
    std::set<int> s1, s2;
    const int64_t mask = (int64_t)slots - 1;
    for (int k = 0; k < n; k++) {
        const int64_t rot = (int64_t)diags[k] & mask;
        const int idxN1 = (int)(((rot / N1) * N1) & mask), idxN2 = (int)(rot & ((int64_t)N1 - 1));
        out.index[idxN1].push_back(idxN2);
        s1.insert(idxN1);
        s2.insert(idxN2);
    }
    for (auto &kv : out.index) std::sort(kv.second.begin(), kv.second.end());
    out.rotN1.assign(s1.begin(), s1.end());
    out.rotN2.assign(s2.begin(), s2.end());
    return out;
}
// float64(a) / float64(b) with the IEEE 754 results of a zero divisor spelled out
inline double ratio_f64(int a, int b) {
    if (b != 0) return (double)a / (double)b;
    if (a > 0) return std::numeric_limits<double>::infinity();
    if (a < 0) return -std::numeric_limits<double>::infinity();
    return std::numeric_limits<double>::quiet_NaN();
}
// FindBestBSGSRatio (lintrans.go:321)
inline int find_best_bsgs_ratio(const int *diags, int n, int maxN, int logMaxRatio) {
    const double maxRatio = (double)((int64_t)1 << logMaxRatio);
    for (int64_t N1 = 1; N1 < maxN; N1 <<= 1) {
        const BsgsIndex ix = bsgs_index(diags, n, maxN, (int)N1);
        const double r = ratio_f64((int)ix.rotN2.size() - 1, (int)ix.rotN1.size() - 1);
        if (r == maxRatio) return (int)N1;
        if (r > maxRatio) return (int)(N1 / 2);
    }
    return 1;
}
// GaloisElements (lintrans.go:297)
inline std::vector<uint64_t> galois_elements(uint64_t nth_root, const int *diags, int n, int slots, int logBSGSRatio) {
    std::vector<uint64_t> out;
    if (logBSGSRatio < 0) {
        for (int r : bsgs_index(diags, n, slots, slots).rotN2) out.push_back(galois_element(nth_root, r));
        return out;
    }
    const int N1 = find_best_bsgs_ratio(diags, n, slots, logBSGSRatio);
    const BsgsIndex ix = bsgs_index(diags, n, slots, N1 > 0 ? N1 : 1);
    std::set<int> u(ix.rotN1.begin(), ix.rotN1.end());
    u.insert(ix.rotN2.begin(), ix.rotN2.end());
    for (int r : u) out.push_back(galois_element(nth_root, r));
    return out;
}

// One launch of the grouped kernel per ring part: the members' inner sums over the union of their baby steps.
struct Group {
    std::vector<int> giants;  // the members j, ascending (at most G)
    std::vector<int> babies;  // the union of the members' baby steps i, ascending
    std::vector<int> term;    // [babies.size()][giants.size()]: position of diagonal j + i in the input list, or -1 (absent)
};
struct Plan {
    int N1 = 0, G = 1;
    std::vector<Group> groups;     // BSGS form; empty in the naive form
    std::vector<int> babies;       // BSGS: every baby step of the transformation, ascending (the pre-rotations it reads)
    std::vector<int> rotations;    // naive form: the non-zero rotations, ascending
    std::vector<int> rotation_term;  // ... and the position of each one's diagonal in the input list
    int zero_diag = -1;            // naive form: position of the zero diagonal, or -1
    std::vector<uint64_t> galois;  // what the call asks the key set for: BSGS the non-zero baby steps then the non-zero giant
                                   // steps, naive the non-zero rotations
    size_t n_giants() const { size_t n = 0; for (const Group &g : groups) n += g.giants.size(); return n; }
};
// diags: the REDUCED diagonal indices (in [0, slots), no duplicates), slots a power of two, N1 = 0 (naive) or a power of two,
// G in [1, kMaxGroup].  false on an argument outside that.
inline bool build_plan(const int *diags, int n, int slots, int N1, int G, uint64_t nth_root, Plan *out) {
    if (!out || n < 0 || (n > 0 && !diags) || slots < 1 || (slots & (slots - 1)) || N1 < 0 || (N1 & (N1 - 1)) || G < 1 || G > kMaxGroup ||
        nth_root < 2 || (nth_root & (nth_root - 1)))
        return false;
    std::map<int, int> pos;
    for (int k = 0; k < n; k++) {
        if (diags[k] < 0 || diags[k] >= slots || pos.count(diags[k])) return false;
        pos[diags[k]] = k;
    }
    Plan p;
    p.N1 = N1; p.G = G;
    if (N1 == 0) {
        for (const auto &kv : pos) {
            if (kv.first == 0) { p.zero_diag = kv.second; continue; }
            p.rotations.push_back(kv.first);
            p.rotation_term.push_back(kv.second);
            p.galois.push_back(galois_element(nth_root, kv.first));
        }
        *out = std::move(p);
        return true;
    }
    const BsgsIndex ix = bsgs_index(diags, n, slots, N1);
    p.babies = ix.rotN2;
    for (size_t g0 = 0; g0 < ix.rotN1.size(); g0 += (size_t)G) {
        Group grp;
        std::set<int> u;
        for (size_t m = g0; m < std::min(ix.rotN1.size(), g0 + (size_t)G); m++) {
            grp.giants.push_back(ix.rotN1[m]);
            const std::vector<int> &b = ix.index.at(ix.rotN1[m]);
            u.insert(b.begin(), b.end());
        }
        grp.babies.assign(u.begin(), u.end());
        grp.term.assign(grp.babies.size() * grp.giants.size(), -1);
        for (size_t s = 0; s < grp.babies.size(); s++)
            for (size_t m = 0; m < grp.giants.size(); m++) {
                const auto it = pos.find(grp.giants[m] + grp.babies[s]);
                // (a diagonal j' + i' of ANOTHER giant step never equals j + i: i, i' < N1 and j, j' are multiples of N1)
                if (it != pos.end()) grp.term[s * grp.giants.size() + m] = it->second;
            }
        p.groups.push_back(std::move(grp));
    }
    for (int i : ix.rotN2) if (i != 0) p.galois.push_back(galois_element(nth_root, i));
    for (int j : ix.rotN1) if (j != 0) p.galois.push_back(galois_element(nth_root, j));
    *out = std::move(p);
    return true;
}
// the plan as words (he_debug_lintrans_plan): n_groups, n_galois, then per group n_members, n_babies, the members, the babies and
// term[n_babies][n_members]; then the Galois elements.  Naive form: n_groups = 0, n_galois, zero_diag, then the elements.
inline std::vector<int64_t> plan_words(const Plan &p) {
    std::vector<int64_t> w;
    w.push_back((int64_t)p.groups.size());
    w.push_back((int64_t)p.galois.size());
    if (p.N1 == 0) w.push_back(p.zero_diag);
    for (const Group &g : p.groups) {
        w.push_back((int64_t)g.giants.size());
        w.push_back((int64_t)g.babies.size());
        for (int j : g.giants) w.push_back(j);
        for (int i : g.babies) w.push_back(i);
        for (int t : g.term) w.push_back(t);
    }
    for (uint64_t e : p.galois) w.push_back((int64_t)e);
    return w;
}
}  // namespace lintrans
