// The structure of a polynomial evaluation on a ciphertext (circuits/common/polynomial), decided on the host: which powers are
// made, from which, relinearized and rescaled when; into which baby-step polynomials ("leaves") the Paterson-Stockmeyer
// decomposition cuts the polynomial, at which level each is evaluated and over which powers; and in which order the leaves are
// combined.  All of it is integer logic over (degree, basis, parity, lazy, input level, powers present).  Scales and coefficient
// values are not the plan's business: the language mirrors, where the scales of MulRelin and Rescale live, supply the numbers.
// Host only, no HIP or library includes: tests/cpp/polyeval_plan_test.cpp runs it on the CPU.
//
// The reference's behaviour, reproduced:
//  - bignum.OptimalSplit (utils/bignum/polynomial.go:14-24) and SplitDegree (power_basis.go:31-49).
//  - Evaluate (polynomial_evaluator.go:33-99): X^1 is a copy of the input; the largest power of two below the degree is made
//    without lazy relinearization, then the powers 2^logSplit - 1 ... 3 the parity keeps, lazily when the polynomial says so.
//  - GenPower / genPower (power_basis.go:76-160): X^n = X^a X^b; with lazy set a power that is no power of two keeps degree 2 and
//    its operands are relinearized first; a power made now is rescaled by whoever uses it next (or by GenPower itself at the top);
//    Chebyshev: T_n = 2 T_a T_b - T_|a-b|, the constant -1 when a == b.
//  - recursePS (polynomial.go:88-141): a polynomial of degree below 2^logSplit is a leaf, unless it leads and its MaxDeg calls for
//    the re-split with OptimalSplit; otherwise it is cut at the power of two 2^logSplit <= n with n >= (deg >> 1) + 1, the
//    quotient one level above the remainder.  A leaf's level does not depend on any scale.
//  - EvaluatePolynomialVectorFromPowerBasis (:254-359): a leaf is a new ciphertext of the widest degree among the powers it
//    reads, plus its constant when the polynomial is even (or of no parity), plus c_k X^k for k = deg ... 1 the parity keeps.
//  - EvaluatePatersonStockmeyerPolynomialVector (:101-161) with EvaluateMonomial (:212-251): neighbours of equal degree merge as
//    low + Rescale(Relinearize(high)) * X^(2^k); the result is relinearized and rescaled.
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

namespace polyeval {
enum Basis { kMonomial = 0, kChebyshev = 1 };
// one primitive call of the reference's evaluators, in its order; dst / a / b name a power (n >= 1) or a leaf (-1 - index)
enum Op {
    kCopyNew = 0,      // X^1 = copy of the input
    kRelinearize,      // dst = Relinearize(dst)
    kRescale,          // dst = Rescale(dst)
    kMulNew,           // dst = a * b (degree 2)
    kMulRelinNew,      // dst = Relinearize(a * b)
    kAddSelf,          // dst = dst + dst (Chebyshev)
    kAddMinusOne,      // dst = dst - 1 at dst's scale (Chebyshev, a == b)
    kSub,              // dst = dst - a (Chebyshev)
    kNewCiphertext,    // dst = a zero leaf
    kAddConst,         // dst = dst + c_0
    kMulThenAdd,       // dst = dst + c_k * a
    kMul,              // dst = dst * a (no relinearization)
    kAdd,              // dst = dst + a
    kOpCount
};
struct Step { int op, dst, level, degree, a, b; };
struct Leaf {
    int degree;        // of the baby-step polynomial (its coefficient list has degree + 1 entries)
    int level;         // the level it is evaluated at
    int new_degree;    // ciphertext degree it is allocated with: the widest power it could read
    int ct_degree;     // ciphertext degree of its result: MulThenAdd resizes the accumulator to the degree of each power in turn
                       // (schemes/ckks/evaluator.go:936, schemes/bgv/evaluator.go:1118), so that of the lowest power it uses
    bool lead;
    uint32_t present;  // bit k: it has term k (bit 0: the constant)
};
struct Power { int level, degree; };
struct Plan {
    int log_degree = 0, log_split = 0, depth = 0;
    std::vector<Step> steps;
    std::vector<Leaf> leaves;
    std::map<int, Power> powers;  // as they stand after the evaluation
    int out_level = 0;
    int result = 0;               // the leaf that holds the result (-1 - index)
    std::string error;            // non-empty: the evaluation is refused
};

inline int bit_len(uint64_t n) { int b = 0; for (; n; n >>= 1) b++; return b; }

inline int optimal_split(int log_degree) {
    int s = log_degree >> 1;
    const int rest = log_degree - s;
    const int64_t here = ((int64_t)1 << s) + ((int64_t)1 << rest) + rest - 3;
    // (rest >= 1 for every log_degree >= 1; log_degree 0 has rest 0 and the reference's 1 << -1 panics: answered with 0)
    if (rest < 1) return s;
    const int64_t next = ((int64_t)1 << (s + 1)) + ((int64_t)1 << (rest - 1)) + rest - 4;
    return here > next ? s + 1 : s;
}
inline void split_degree(int n, int *a, int *b) {
    if ((n & (n - 1)) == 0) { *a = *b = n >> 1; return; }
    const int top = 1 << (bit_len((uint64_t)n - 1) - 1);
    *a = top - 1; *b = n + 1 - top;
}
// the levels an evaluation of this degree consumes: ceil(log2 degree)
inline int depth_of(int degree) { return degree > 1 ? bit_len((uint64_t)degree - 1) : 0; }
inline bool wanted(int i, bool even, bool odd) { return (!even && !odd) ? true : ((i & 1) == 0 ? even : odd); }

namespace detail {
struct Builder {
    Plan &P;
    int basis;
    void push(int op, int dst, int level, int degree, int a = 0, int b = 0) { P.steps.push_back(Step{op, dst, level, degree, a, b}); }
    void relin(int n) { Power &x = P.powers[n]; x.degree = 1; push(kRelinearize, n, x.level, x.degree); }
    void rescale(int n) { Power &x = P.powers[n]; x.level -= 1; push(kRescale, n, x.level, x.degree); }
    bool build(int m, bool lz) {
        if (P.powers.count(m)) return false;
        int a, b;
        split_degree(m, &a, &b);
        const bool pow2 = (m & (m - 1)) == 0;
        const bool owe_a = build(a, lz && !pow2);
        const bool owe_b = build(b, lz && !pow2);
        if (lz) {
            if (P.powers[a].degree == 2) relin(a);
            if (P.powers[b].degree == 2) relin(b);
        }
        if (owe_a) rescale(a);
        if (owe_b) rescale(b);
        const Power xa = P.powers[a], xb = P.powers[b];
        Power xm{xa.level < xb.level ? xa.level : xb.level, lz ? xa.degree + xb.degree : 1};
        P.powers[m] = xm;
        push(lz ? kMulNew : kMulRelinNew, m, xm.level, xm.degree, a, b);
        if (basis == kChebyshev) {
            const int gap = a > b ? a - b : b - a;
            push(kAddSelf, m, xm.level, xm.degree, m, m);
            if (gap == 0) push(kAddMinusOne, m, xm.level, xm.degree);
            else {
                grow(gap, lz);
                const Power xg = P.powers[gap];
                Power &r = P.powers[m];
                if (xg.level < r.level) r.level = xg.level;
                if (xg.degree > r.degree) r.degree = xg.degree;
                push(kSub, m, r.level, r.degree, gap);
            }
        }
        return true;
    }
    void grow(int n, bool lazy) {
        if (P.powers.count(n)) return;
        if (build(n, lazy)) rescale(n);
    }
};
struct Sub {  // a polynomial of the decomposition: only its length and metadata matter here
    int degree, maxdeg;
    bool lead;
};
}  // namespace detail

// GenPower alone on a basis (`powers`: what it holds, X^1 included); the steps are appended to P
inline void gen_power(Plan &P, int basis, int n, bool lazy) {
    detail::Builder B{P, basis};
    B.grow(n, lazy);
}

// The whole evaluation.  present: the powers the basis already holds (n -> level, degree); it must hold X^1.  copy_input: the
// call is Evaluate on a ciphertext (X^1 is copied first) and not EvaluateFromPowerBasis.
inline Plan build_plan(int degree, int basis, bool even, bool odd, bool lazy, const std::map<int, Power> &present, bool copy_input) {
    Plan P;
    P.powers = present;
    if (degree < 1) { P.error = "the polynomial must have degree >= 1"; return P; }
    if (basis != kMonomial && basis != kChebyshev) { P.error = "unknown basis"; return P; }
    if (!P.powers.count(1)) { P.error = "cannot EvaluateFromPowerBasis: X^{1} is nil"; return P; }
    const int level = P.powers[1].level;
    P.depth = depth_of(degree);
    P.log_degree = bit_len((uint64_t)degree);
    P.log_split = optimal_split(P.log_degree);
    if (level < P.depth) {
        P.error = std::to_string(level) + " levels < " + std::to_string(P.depth) + " log(d) -> cannot evaluate poly";
        return P;
    }
    detail::Builder B{P, basis};
    if (copy_input) B.push(kCopyNew, 1, level, P.powers[1].degree);
    B.grow(1 << (P.log_degree - 1), false);
    for (int i = (1 << P.log_split) - 1; i > 2; i--)
        if (wanted(i, even, odd)) B.grow(i, lazy);
    // recursePS: the leaves, quotients before remainders
    struct Rec {
        Plan &P; bool even, odd;
        void leaf(const detail::Sub &p, int lvl) {
            Leaf f{p.degree, lvl, 1, 1, p.lead, 0};
            if (even) f.present |= 1u;
            const int low = (even && !odd) ? p.degree - 1 : p.degree;
            if (low != 0) {
                int widest = 0;
                for (int k = p.degree; k > 0; k--) {
                    auto it = P.powers.find(k);
                    if (it != P.powers.end() && it->second.degree > widest) widest = it->second.degree;
                    if (wanted(k, even, odd)) {
                        if (k < 32) f.present |= 1u << k;
                        if (it == P.powers.end() && P.error.empty()) P.error = "a leaf needs X^{" + std::to_string(k) + "}, which the basis lacks";
                    }
                }
                f.new_degree = f.ct_degree = widest;
                for (int k = p.degree; k > 0; k--)
                    if (wanted(k, even, odd) && P.powers.count(k)) f.ct_degree = P.powers[k].degree;
            }
            if (p.degree > 31 && P.error.empty()) P.error = "a baby step of more than 31 terms";
            P.leaves.push_back(f);
        }
        void descend(const detail::Sub &p, int ls, int lvl) {
            if (p.degree < (1 << ls)) {
                if (p.lead && ls > 1 && p.maxdeg > (1 << bit_len((uint64_t)p.maxdeg)) - (1 << (ls - 1))) {
                    descend(p, optimal_split(bit_len((uint64_t)p.degree)), lvl);
                    return;
                }
                leaf(p, lvl);
                return;
            }
            int step = 1 << ls;
            while (step < (p.degree >> 1) + 1) step <<= 1;
            const detail::Sub q{p.degree - step, p.maxdeg, p.lead};
            const detail::Sub r{step - 1, p.maxdeg == p.degree ? step - 1 : p.maxdeg - (p.degree - step + 1), false};
            descend(q, ls, lvl + 1);
            descend(r, ls, lvl);
        }
    } R{P, even, odd};
    R.descend(detail::Sub{degree, degree, true}, P.log_split, level - (P.log_degree - 1));
    if (!P.error.empty()) return P;
    // the baby steps
    const int n = (int)P.leaves.size();
    std::vector<Power> ct(n);
    for (int i = 0; i < n; i++) {
        const Leaf &f = P.leaves[i];
        const int id = -1 - i;
        ct[i] = Power{f.level, f.ct_degree};
        B.push(kNewCiphertext, id, f.level, f.new_degree);
        if (f.present & 1u) B.push(kAddConst, id, f.level, f.new_degree);
        for (int k = f.degree; k > 0; k--)
            if ((f.present >> k) & 1u) B.push(kMulThenAdd, id, f.level, P.powers[k].degree, k);
    }
    // the giant steps: parts in the reversed order of the leaves
    struct Part { int degree, leaf; };
    std::vector<Part> parts(n);
    for (int i = 0; i < n; i++) parts[n - 1 - i] = Part{P.leaves[i].degree, i};
    while (parts.size() > 1) {
        const int np = (int)parts.size();
        std::vector<int> action(np, 0);
        for (int i = 0; i < np; i++) {
            if (i == np - 1) action[i] = 2;
            else if (parts[i].degree == parts[i + 1].degree) { action[i] = 1; i++; }
        }
        std::vector<bool> gone(np, false);
        for (int i = 0; i < np; i++) {
            if (action[i] == 2) parts[i].degree = parts[i - 1].degree;
            else if (action[i] == 1) {
                const int low = parts[i].leaf, high = parts[i + 1].leaf;
                const int width = 1 << bit_len((uint64_t)parts[i].degree);
                if (!P.powers.count(width)) { P.error = "the giant steps need X^{" + std::to_string(width) + "}, which the basis lacks"; return P; }
                Power &hv = ct[high];
                const Power xv = P.powers[width];
                if (hv.degree == 2) { hv.degree = 1; B.push(kRelinearize, -1 - high, hv.level, hv.degree); }
                hv.level -= 1;
                B.push(kRescale, -1 - high, hv.level, hv.degree);
                if (xv.level < hv.level) hv.level = xv.level;
                hv.degree += xv.degree;
                B.push(kMul, -1 - high, hv.level, hv.degree, width);
                if (ct[low].level < hv.level) hv.level = ct[low].level;
                if (ct[low].degree > hv.degree) hv.degree = ct[low].degree;
                B.push(kAdd, -1 - high, hv.level, hv.degree, -1 - low);
                parts[i + 1].degree = 2 * width - 1;
                gone[i] = true;
            }
        }
        std::vector<Part> next;
        for (int i = 0; i < np; i++)
            if (!gone[i]) next.push_back(parts[i]);
        parts.swap(next);
    }
    const int res = parts[0].leaf;
    if (ct[res].degree == 2) { ct[res].degree = 1; B.push(kRelinearize, -1 - res, ct[res].level, 1); }
    ct[res].level -= 1;
    B.push(kRescale, -1 - res, ct[res].level, ct[res].degree);
    P.result = -1 - res;
    P.out_level = ct[res].level;
    return P;
}

// the plan as words (he_debug_polyeval_plan): log_split, depth, n_leaves, n_steps, out_level, then per leaf (degree, level,
// new_degree, ct_degree, present) and per step (op, dst, level, degree, a, b)
inline std::vector<int64_t> plan_words(const Plan &P) {
    std::vector<int64_t> w{P.log_split, P.depth, (int64_t)P.leaves.size(), (int64_t)P.steps.size(), P.out_level};
    for (const Leaf &f : P.leaves) { w.push_back(f.degree); w.push_back(f.level); w.push_back(f.new_degree); w.push_back(f.ct_degree); w.push_back(f.present); }
    for (const Step &s : P.steps) { w.push_back(s.op); w.push_back(s.dst); w.push_back(s.level); w.push_back(s.degree); w.push_back(s.a); w.push_back(s.b); }
    return w;
}
}  // namespace polyeval
