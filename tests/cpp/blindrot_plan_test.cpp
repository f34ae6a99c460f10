// lattigo_amd/csrc/blindrot_plan.h on the CPU: the schedule of one row and the merger of a batch, checked against the properties
// the launch code relies on.  Host only: needs neither the library nor a device, and may be built with the host sanitizers.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "blindrot_plan.h"

using namespace blindrot;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        g_checks++;                                                          \
        if (!(cond)) {                                                       \
            g_failed++;                                                      \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
        }                                                                    \
    } while (0)

// the exponent walk of Algorithm 3 (eprint 2022/198): the accumulator holds X^e; an external product with key j adds s[j], an
// automorphism by g multiplies e by g.  With the reference's schedule the result is sum_i a'[i] s[i] mod 2N, a'[i] = a[i] except
// that 0, 1 and 2N - 1 all count as 1 (set 0 is served after the last automorphism, with no sign).
static uint64_t walk(int logN, const std::vector<Op> &ops, const std::vector<uint64_t> &s) {
    const uint64_t mask = ((uint64_t)2 << logN) - 1;
    uint64_t e = 0;
    for (const Op &op : ops) {
        if (op.kind == OP_EXTERNAL_PRODUCT) e = (e + s[op.arg]) & mask;
        else e = (e * op.arg) & mask;
    }
    return e;
}

static void check_row(int logN, const std::vector<uint64_t> &a, std::mt19937_64 &rng) {
    const uint64_t twoN = (uint64_t)2 << logN, mask = twoN - 1;
    std::vector<Op> ops;
    CHECK(blindrot_ops(logN, a.data(), (int)a.size(), &ops));
    // every key exactly once; every Galois element one of g^1..g^10, 2N - g
    std::vector<int> seen(a.size(), 0);
    const std::vector<uint64_t> gals = galois_elements(logN);
    size_t n_minus_g = 0;
    for (const Op &op : ops) {
        if (op.kind == OP_EXTERNAL_PRODUCT) {
            CHECK(op.arg < a.size());
            if (op.arg < a.size()) seen[op.arg]++;
        } else {
            bool known = false;
            for (uint64_t g : gals) known = known || g == op.arg;
            CHECK(known);
            n_minus_g += op.arg == twoN - kGaloisGen;
        }
    }
    for (int c : seen) CHECK(c == 1);
    CHECK(n_minus_g >= 1);
    // the walk in the exponent
    std::vector<uint64_t> s(a.size());
    for (uint64_t &x : s) x = rng() & mask;
    uint64_t want = 0;
    for (size_t i = 0; i < a.size(); i++) {
        const uint64_t ai = (a[i] == 0 || a[i] == twoN - 1) ? 1 : a[i];
        want = (want + ai * s[i]) & mask;
    }
    CHECK(walk(logN, ops, s) == want);
}

int main() {
    std::mt19937_64 rng(0x1A77160);
    for (int logN = 4; logN <= 11; logN++) {
        const uint64_t twoN = (uint64_t)2 << logN, N = twoN >> 1;
        for (int n_lwe : {1, 3, 16, 64}) {
            for (int rep = 0; rep < 4; rep++) {
                std::vector<uint64_t> a((size_t)n_lwe);
                for (uint64_t &x : a) x = (rng() % N) * 2 + 1;
                check_row(logN, a, rng);
            }
            std::vector<uint64_t> same((size_t)n_lwe, (rng() % N) * 2 + 1);
            check_row(logN, same, rng);
        }
        // 0, 1 and 2N - 1 share set 0: the three products are the last operations
        std::vector<uint64_t> a = {0, 1, twoN - 1, 5, twoN - 5};
        check_row(logN, a, rng);
        std::vector<Op> ops;
        CHECK(blindrot_ops(logN, a.data(), (int)a.size(), &ops));
        CHECK(ops.size() >= 3 && ops[ops.size() - 3].kind == OP_EXTERNAL_PRODUCT && ops[ops.size() - 3].arg == 0 &&
              ops[ops.size() - 2].arg == 1 && ops[ops.size() - 1].arg == 2 && ops[ops.size() - 1].kind == OP_EXTERNAL_PRODUCT);
        // k = 1 forces its automorphism; a[i] = g^1 is served just before it
        // a non-zero even word, and a word outside [0, 2N)
        std::vector<Op> keep = ops;
        std::vector<uint64_t> bad = {1, 6, 3};
        CHECK(!blindrot_ops(logN, bad.data(), 3, &ops));
        CHECK(ops.size() == keep.size());
        bad[1] = twoN + 1;
        CHECK(!blindrot_ops(logN, bad.data(), 3, &ops));
    }
    CHECK(galois_element(10, 1) == 5 && galois_element(10, 3) == 125 && galois_element(9, 10) == (9765625u & 1023u));
    // the merger: every entry's subsequence is its own list; as many rounds as the longest entry alone
    for (int logN : {5, 9, 10}) {
        const uint64_t N = (uint64_t)1 << logN;
        std::vector<std::vector<Op>> lists(5);
        size_t longest = 0;
        for (size_t b = 0; b < lists.size(); b++) {
            std::vector<uint64_t> a(b == 2 ? 1 : 16);
            for (uint64_t &x : a) x = b == 3 ? 7 : (rng() % N) * 2 + 1;
            CHECK(blindrot_ops(logN, a.data(), (int)a.size(), &lists[b]));
            longest = std::max(longest, blindrot_round_count(lists[b]));
        }
        const std::vector<Round> rounds = blindrot_merge(lists);
        CHECK(rounds.size() == longest);
        for (size_t b = 0; b < lists.size(); b++) {
            std::vector<Op> got;
            for (const Round &r : rounds) {
                CHECK(r.gal.size() == lists.size() && r.prod.size() == lists.size());
                if (r.gal[b]) got.push_back(Op{OP_AUTOMORPHISM, r.gal[b]});
                if (r.prod[b] >= 0) got.push_back(Op{OP_EXTERNAL_PRODUCT, (uint64_t)r.prod[b]});
            }
            CHECK(got.size() == lists[b].size());
            for (size_t i = 0; i < got.size() && i < lists[b].size(); i++) CHECK(got[i].kind == lists[b][i].kind && got[i].arg == lists[b][i].arg);
        }
    }
    CHECK(blindrot_merge({}).empty());
    std::printf("%s: %d checks, %d failed\n", g_failed ? "FAIL" : "PASS", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
