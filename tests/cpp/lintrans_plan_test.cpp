// lattigo_amd/csrc/lintrans_plan.h on the CPU: the index of a linear transformation and the grouping of its giant steps, checked
// against the properties the launch code relies on.  Host only: needs neither the library nor a device, and may be built with the
// host sanitizers.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

#include "lintrans_plan.h"

using namespace lintrans;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        g_checks++;                                                          \
        if (!(cond)) {                                                       \
            g_failed++;                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
        }                                                                    \
    } while (0)

// every diagonal is a term of exactly one (group, baby step, member); the members of all groups are the sorted giant steps, at
// most G per group and only the last group short; a group's baby steps are the sorted union of its members'; term positions
// name the diagonal j + i; the Galois list is the non-zero baby steps, then the non-zero giant steps
static void check_plan(const std::vector<int> &diags, int slots, int N1, int G, uint64_t nth) {
    Plan p;
    CHECK(build_plan(diags.data(), (int)diags.size(), slots, N1, G, nth, &p));
    const BsgsIndex ix = bsgs_index(diags.data(), (int)diags.size(), slots, N1);
    std::vector<int> giants;
    std::vector<int> used(diags.size(), 0);
    for (size_t g = 0; g < p.groups.size(); g++) {
        const Group &grp = p.groups[g];
        CHECK(!grp.giants.empty() && (int)grp.giants.size() <= G);
        CHECK(g + 1 == p.groups.size() || (int)grp.giants.size() == G);
        CHECK(grp.term.size() == grp.babies.size() * grp.giants.size());
        CHECK(std::is_sorted(grp.babies.begin(), grp.babies.end()) && std::is_sorted(grp.giants.begin(), grp.giants.end()));
        std::set<int> u;
        for (int j : grp.giants) {
            giants.push_back(j);
            CHECK(j % N1 == 0);
            const auto it = ix.index.find(j);
            CHECK(it != ix.index.end());
            if (it != ix.index.end()) u.insert(it->second.begin(), it->second.end());
        }
        CHECK(std::vector<int>(u.begin(), u.end()) == grp.babies);
        for (size_t s = 0; s < grp.babies.size(); s++) {
            bool any = false;
            for (size_t m = 0; m < grp.giants.size(); m++) {
                const int t = grp.term[s * grp.giants.size() + m];
                if (t < 0) continue;
                any = true;
                CHECK(t < (int)diags.size());
                if (t < (int)diags.size()) {
                    CHECK(diags[(size_t)t] == grp.giants[m] + grp.babies[s]);
                    used[(size_t)t]++;
                }
            }
            CHECK(any);  // a baby step is in the union because some member has it
        }
    }
    CHECK(giants == ix.rotN1);
    CHECK(p.n_giants() == ix.rotN1.size());
    for (int u : used) CHECK(u == 1);
    CHECK(p.babies == ix.rotN2);
    std::vector<uint64_t> want;
    for (int i : ix.rotN2) if (i) want.push_back(galois_element(nth, i));
    for (int j : ix.rotN1) if (j) want.push_back(galois_element(nth, j));
    CHECK(p.galois == want);
    const std::vector<int64_t> w = plan_words(p);
    CHECK(w.size() >= 2 && w[0] == (int64_t)p.groups.size() && w[1] == (int64_t)p.galois.size());
}

int main() {
    std::mt19937_64 rng(20251);
    // GaloisGen^k mod NthRoot, negative rotations included
    CHECK(galois_element(2048, 0) == 1 && galois_element(2048, 1) == 5 && galois_element(2048, 2) == 25);
    CHECK(galois_element(2048, -1) * 5 % 2048 == 1);
    CHECK(galois_element(4096, 3) == 125);
    // BSGSIndex: the reduction of negative and out-of-range rotations
    {
        const std::vector<int> d = {-1, 5, 517, 0};
        const BsgsIndex ix = bsgs_index(d.data(), 4, 512, 4);
        CHECK((ix.rotN1 == std::vector<int>{0, 4, 508}));
        CHECK((ix.rotN2 == std::vector<int>{0, 1, 3}));
        CHECK((ix.index.at(4) == std::vector<int>{1, 1}));
    }
    // the float64 comparisons with a zero count
    CHECK(std::isinf(ratio_f64(3, 0)) && ratio_f64(3, 0) > 0 && std::isinf(ratio_f64(-1, 0)) && ratio_f64(-1, 0) < 0);
    CHECK(std::isnan(ratio_f64(0, 0)) && !(ratio_f64(0, 0) == 1.0) && !(ratio_f64(0, 0) > 1.0));
    {
        const std::vector<int> one = {5}, none, four = {0, 1, 2, 3}, sixteen = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
        CHECK(find_best_bsgs_ratio(one.data(), 1, 64, 2) == 1);     // NaN at every N1: the walk ends, 1
        CHECK(find_best_bsgs_ratio(none.data(), 0, 16, 1) == 1);    // (-1) / (-1) = 1 != 2, never greater
        CHECK(find_best_bsgs_ratio(four.data(), 4, 64, 0) == 2);    // 1 / 1 == 1 at N1 = 2
        CHECK(find_best_bsgs_ratio(sixteen.data(), 16, 512, 0) == 4);  // 3 / 3 at N1 = 4
        CHECK(find_best_bsgs_ratio(sixteen.data(), 16, 512, 1) == 4);  // 7 / 1 > 2 at N1 = 8: N1 / 2
        CHECK(galois_elements(2048, four.data(), 4, 512, -1).size() == 4);  // naive: every rotation, the zero one included
        CHECK(galois_elements(2048, four.data(), 4, 512, 0).size() == 3);   // N1 = 2: {0, 2} and {0, 1}
    }
    // the plans of the launch code
    const std::vector<std::vector<int>> fixed = {{0, 1, 2, 3, 8, 9, 17, 18, 26, 35, 41}, {0, 8, 16, 24, 32}, {1, 2, 9, 17, 18},
                                                 {5, 6, 13, 14}, {1, 2, 3}, {0}, {7}};
    for (const auto &d : fixed)
        for (int G = 1; G <= kMaxGroup; G++) check_plan(d, 512, 8, G, 2048);
    {
        std::vector<int> many;  // more than 64 baby steps in one giant step, more than 64 terms in a group
        for (int i = 0; i < 300; i += (i < 70 ? 1 : 3)) many.push_back(i);
        for (int G : {1, 2, 4}) check_plan(many, 512, 128, G, 4096);
    }
    for (int round = 0; round < 200; round++) {
        const int logs = 3 + (int)(rng() % 10), slots = 1 << logs, N1 = 1 << (rng() % (uint64_t)(logs + 1));
        std::set<int> s;
        const int cnt = 1 + (int)(rng() % 60);
        for (int k = 0; k < cnt; k++) s.insert((int)(rng() % (uint64_t)slots));
        check_plan(std::vector<int>(s.begin(), s.end()), slots, N1, 1 + (int)(rng() % 4), (uint64_t)4 << logs);
    }
    // the naive form
    {
        const std::vector<int> d = {130, 0, 3, 1};
        Plan p;
        CHECK(build_plan(d.data(), 4, 512, 0, 1, 2048, &p));
        CHECK(p.groups.empty() && p.zero_diag == 1 && (p.rotations == std::vector<int>{1, 3, 130}) && (p.rotation_term == std::vector<int>{3, 2, 0}));
        CHECK(p.galois.size() == 3 && p.galois[0] == 5);
    }
    // arguments it refuses: `out` stays as it was
    {
        Plan p;
        p.G = 77;
        const std::vector<int> dup = {1, 1}, big = {512}, neg = {-1}, ok = {1};
        CHECK(!build_plan(dup.data(), 2, 512, 4, 1, 2048, &p) && !build_plan(big.data(), 1, 512, 4, 1, 2048, &p));
        CHECK(!build_plan(neg.data(), 1, 512, 4, 1, 2048, &p) && !build_plan(ok.data(), 1, 500, 4, 1, 2048, &p));
        CHECK(!build_plan(ok.data(), 1, 512, 3, 1, 2048, &p) && !build_plan(ok.data(), 1, 512, 4, 0, 2048, &p));
        CHECK(!build_plan(ok.data(), 1, 512, 4, kMaxGroup + 1, 2048, &p) && !build_plan(ok.data(), 1, 512, 4, 1, 2047, &p));
        CHECK(!build_plan(nullptr, 1, 512, 4, 1, 2048, &p) && !build_plan(ok.data(), 1, 512, 4, 1, 2048, nullptr));
        CHECK(p.G == 77);
        CHECK(build_plan(nullptr, 0, 512, 4, 1, 2048, &p) && p.groups.empty() && p.galois.empty());
    }
    std::printf("%s: %d checks, %d failed\n", g_failed ? "FAIL" : "PASS", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
