// lattigo_amd/csrc/polyeval_plan.h on the CPU: the structure of a polynomial evaluation against closed forms and the properties
// the launch code relies on.  Host only: needs neither the library nor a device, and may be built with the host sanitizers.
#include <cstdio>
#include <cstdlib>
#include <set>

#include "polyeval_plan.h"

using namespace polyeval;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        g_checks++;                                                          \
        if (!(cond)) {                                                       \
            g_failed++;                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
        }                                                                    \
    } while (0)

// the non-scalar multiplications of a Paterson-Stockmeyer evaluation with baby-step width s of a polynomial of ld bits, as
// bignum.OptimalSplit counts them: 2^s + 2^(ld - s) + ld - s - 3
static long cost(int ld, int s) { return (1L << s) + (1L << (ld - s)) + ld - s - 3; }

static void check_helpers() {
    for (int ld = 1; ld <= 30; ld++) {
        const int s = optimal_split(ld);
        CHECK(s == ld / 2 || s == ld / 2 + 1);
        CHECK(cost(ld, s) <= cost(ld, ld / 2) && (ld / 2 + 1 > ld || cost(ld, s) <= cost(ld, ld / 2 + 1) || s == ld / 2));
        // the reference moves to the wider split only where it is strictly cheaper
        CHECK((s == ld / 2 + 1) == (cost(ld, ld / 2) > cost(ld, ld / 2 + 1)));
    }
    for (int n = 1; n < 5000; n++) {
        int a = 0, b = 0;
        split_degree(n, &a, &b);
        CHECK((a + b == n || n == 1) && a >= 0 && b >= 0);  // (the reference's SplitDegree(1) is (0, 0))
        if ((n & (n - 1)) == 0) CHECK(a == b);
        else CHECK(((a + 1) & a) == 0 && a + 1 <= n - 1 && 2 * (a + 1) > n - 1 && b >= 1);  // a = 2^k - 1, the largest such below n
        CHECK(depth_of(n) == (n > 1 ? bit_len((uint64_t)n - 1) : 0));
        CHECK((1L << depth_of(n)) >= n && (n == 1 || (1L << (depth_of(n) - 1)) < n));
    }
    CHECK(wanted(3, false, false) && wanted(4, true, true) && wanted(4, true, false) && !wanted(3, true, false) && !wanted(4, false, true));
}

static void check_plan(int degree, int basis, bool even, bool odd, bool lazy, int level) {
    const std::map<int, Power> in{{1, Power{level, 1}}};
    const Plan p = build_plan(degree, basis, even, odd, lazy, in, true);
    if (level < depth_of(degree)) {
        CHECK(p.error == std::to_string(level) + " levels < " + std::to_string(depth_of(degree)) + " log(d) -> cannot evaluate poly");
        return;
    }
    CHECK(p.error.empty());
    if (!p.error.empty()) return;
    CHECK(p.log_split == optimal_split(bit_len((uint64_t)degree)) && p.depth == depth_of(degree));
    CHECK(p.out_level == level - bit_len((uint64_t)degree));
    // the baby steps partition the coefficients; none is wider than the entry admits; only the first one leads
    long coeffs = 0;
    for (const Leaf &f : p.leaves) {
        coeffs += f.degree + 1;
        CHECK(f.degree >= 0 && f.degree <= 31 && f.degree < (1 << p.log_split));
        CHECK(f.level > p.out_level && f.level <= level);
        CHECK(((f.present & 1u) != 0) == even || (!even && !odd && (f.present & 1u) == 0));
        int lowest = 0;
        for (int k = f.degree; k >= 1; k--)
            if ((f.present >> k) & 1u) {
                CHECK(wanted(k, even, odd) && p.powers.count(k));
                lowest = k;
            }
        CHECK(((uint64_t)f.present >> (f.degree + 1)) == 0);
        if (lowest) CHECK(f.ct_degree == p.powers.at(lowest).degree && f.new_degree >= f.ct_degree);
        else CHECK(f.ct_degree == f.new_degree && f.ct_degree <= 1);
        if (!lazy) CHECK(f.ct_degree <= 1);
    }
    CHECK(coeffs == degree + 1);
    CHECK(p.leaves.front().lead);
    for (size_t i = 1; i < p.leaves.size(); i++) CHECK(!p.leaves[i].lead);
    // the steps: first the input's copy; a power is made once, from powers that exist, and never sinks below level 0; one giant-step
    // multiplication per baby step but one; the last step rescales the result to the promised level
    CHECK(p.steps.front().op == kCopyNew && p.steps.front().dst == 1);
    std::set<int> made{1};
    long muls = 0, leaf_terms = 0, news = 0;
    bool leaves_begun = false;
    for (const Step &s : p.steps) {
        CHECK(s.level >= 0 && s.degree >= 0 && s.degree <= 2 && s.op >= 0 && s.op < kOpCount);
        if (s.op == kMulNew || s.op == kMulRelinNew) {
            CHECK(!leaves_begun && made.count(s.a) && made.count(s.b) && !made.count(s.dst) && s.a + s.b == s.dst);
            CHECK(s.degree == (s.op == kMulNew ? 2 : 1) && (s.op == kMulRelinNew || lazy));
            made.insert(s.dst);
        }
        if (s.op == kAddSelf || s.op == kAddMinusOne || s.op == kSub) CHECK(basis == kChebyshev && made.count(s.dst));
        if (s.op == kSub) CHECK(made.count(s.a));
        if (s.op == kNewCiphertext) { leaves_begun = true; news++; CHECK(s.dst == -(int)news); }
        if (s.op == kMulThenAdd) { leaf_terms++; CHECK(s.dst < 0 && made.count(s.a)); }
        if (s.op == kMul) { muls++; CHECK(s.dst < 0 && made.count(s.a) && (s.a & (s.a - 1)) == 0 && (s.degree == 2 || s.degree == 1)); }  // (1: a baby step of degree 0)
        if (s.op == kAdd) CHECK(s.dst < 0 && s.a < 0 && s.dst != s.a);
    }
    CHECK(news == (long)p.leaves.size() && muls == (long)p.leaves.size() - 1);
    long want_terms = 0;
    for (const Leaf &f : p.leaves)
        for (int k = 1; k <= f.degree; k++) want_terms += (f.present >> k) & 1u;
    CHECK(leaf_terms == want_terms);
    CHECK(p.steps.back().op == kRescale && p.steps.back().dst == p.result && p.steps.back().level == p.out_level && p.steps.back().degree == 1);
    CHECK(made.count(1 << (bit_len((uint64_t)degree) - 1)));
    // a second evaluation on the basis this one leaves makes no power
    const Plan again = build_plan(degree, basis, even, odd, lazy, p.powers, false);
    CHECK(again.error.empty());
    for (const Step &s : again.steps) CHECK(s.dst < 0 || s.op == kRelinearize);
    CHECK(again.leaves.size() == p.leaves.size());
}

int main() {
    check_helpers();
    for (int degree = 1; degree <= 130; degree++)
        for (int basis = 0; basis < 2; basis++)
            for (int parity = 0; parity < 4; parity++)
                for (int lazy = 0; lazy < 2; lazy++) check_plan(degree, basis, parity & 1, (parity & 2) != 0, lazy != 0, 9);
    for (int degree : {255, 256, 257, 511, 1023}) check_plan(degree, kMonomial, true, true, false, 12);
    for (int level = 0; level < 6; level++) check_plan(33, kChebyshev, false, true, false, level);
    {
        const std::map<int, Power> none{{2, Power{5, 1}}};
        CHECK(build_plan(7, kMonomial, true, true, false, none, false).error == "cannot EvaluateFromPowerBasis: X^{1} is nil");
        const std::map<int, Power> one{{1, Power{5, 1}}};
        CHECK(!build_plan(0, kMonomial, true, true, false, one, false).error.empty());
        CHECK(!build_plan(7, 2, true, true, false, one, false).error.empty());
        CHECK(!build_plan(2047, kMonomial, true, true, false, {{1, Power{20, 1}}}, false).error.empty() ||
              build_plan(2047, kMonomial, true, true, false, {{1, Power{20, 1}}}, false).leaves.front().degree <= 31);
    }
    std::printf("%s: %d checks, %d failed\n", g_failed ? "FAIL" : "PASS", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
