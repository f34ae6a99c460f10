// Polynomial evaluation through the compiled mirror (include/hering.hpp, namespace polyeval), on words read from a file and
// written to another (tests/test_cpp_polyeval.py compares them with answers made from the oracle's arithmetic).
//   polyeval_parity --compile-only     exits 0 (the header's new namespace type-checked)
//   polyeval_parity --host IN OUT      no device.  IN: t nq level ncases | Q[nq] | tInvModQ[level + 1] | per case: c xScale outScale
//                                      OUT: OptimalSplit(1..30) | SplitDegree(1..64) pairs | per case: term words [level + 1],
//                                           constant words [level + 1] | the plan of degree 17 at level 7 as words
//   polyeval_parity --evaluate IN OUT  BGV Evaluate as ONE native call.  IN: logN nq np beta degree t B | q[nq] | p[np] | key q words
//                                      [beta][2][nq][N], p words [beta][2][np][N] | leaf count | s0 rows | s1 rows | ct [2][B][nq][N]
//                                      OUT: the result [2][B][out_level + 1][N]
//   polyeval_parity IN OUT             IN: logN nq degree B npowers | q[nq] | leaf count | s0 rows | s1 rows | powers [npowers][2][B][nq][N]
//                                      OUT: per baby step its two components [B][level + 1][N], at G = 1 and again at G = 4
#include <cstdio>
#include <cstring>
#include <vector>

#include "hering.hpp"

using namespace hering;

static std::vector<uint64_t> read_words(const char *path) {
    std::vector<uint64_t> w;
    FILE *f = std::fopen(path, "rb");
    if (!f) throw std::runtime_error("polyeval_parity: cannot open the input file");
    uint64_t buf[4096];
    size_t n;
    while ((n = std::fread(buf, 8, 4096, f)) > 0) w.insert(w.end(), buf, buf + n);
    std::fclose(f);
    return w;
}
static std::vector<uint64_t> take(const std::vector<uint64_t> &w, size_t &at, size_t n) {
    if (at + n > w.size()) throw std::runtime_error("polyeval_parity: input file too short");
    std::vector<uint64_t> v(w.begin() + at, w.begin() + at + n);
    at += n;
    return v;
}
static void write_words(const char *path, const std::vector<uint64_t> &v) {
    FILE *f = std::fopen(path, "wb");
    if (!f) throw std::runtime_error("polyeval_parity: cannot open the output file");
    std::fwrite(v.data(), 8, v.size(), f);
    std::fclose(f);
}

static int host(const char *in, const char *out) {
    const std::vector<uint64_t> w = read_words(in);
    size_t at = 0;
    const std::vector<uint64_t> hd = take(w, at, 4);
    const int nq = (int)hd[1], level = (int)hd[2], ncases = (int)hd[3];
    const polyeval::BGVWords bw{hd[0], take(w, at, (size_t)nq)};
    const std::vector<uint64_t> tinv = take(w, at, (size_t)level + 1);
    std::vector<uint64_t> o;
    for (int ld = 1; ld <= 30; ld++) o.push_back((uint64_t)polyeval::OptimalSplit(ld));
    for (int n = 1; n <= 64; n++) {
        const auto ab = polyeval::SplitDegree(n);
        o.push_back((uint64_t)ab.first);
        o.push_back((uint64_t)ab.second);
    }
    for (int i = 0; i < ncases; i++) {
        const std::vector<uint64_t> c = take(w, at, 3);
        for (uint64_t x : bw.term(level, c[0], c[1], c[2])) o.push_back(x);
        for (uint64_t x : bw.constant(level, c[0], c[2], tinv)) o.push_back(x);
    }
    const polyeval::Plan plan(17, HE_POLYEVAL_MONOMIAL, true, true, false, {{1, 7, 1}}, true);
    o.push_back((uint64_t)plan.log_split); o.push_back((uint64_t)plan.depth); o.push_back(plan.leaves.size()); o.push_back(plan.steps.size());
    o.push_back((uint64_t)plan.out_level);
    for (const polyeval::LeafInfo &f : plan.leaves) for (int64_t x : {(int64_t)f.degree, (int64_t)f.level, (int64_t)f.new_degree, (int64_t)f.ct_degree, (int64_t)f.present}) o.push_back((uint64_t)x);
    for (const polyeval::Step &s : plan.steps) for (int x : {s.op, s.dst, s.level, s.degree, s.a, s.b}) o.push_back((uint64_t)(int64_t)x);
    // the reference's refusals arrive as exceptions with its messages
    bool threw = false;
    try { polyeval::Depth(9, 3); } catch (const Error &e) { threw = std::strstr(e.what(), "3 levels < 4 log(d) -> cannot evaluate poly") != nullptr; }
    if (!threw) throw std::runtime_error("polyeval_parity: the depth check did not refuse");
    if (polyeval::Depth(9, 4) != 4) throw std::runtime_error("polyeval_parity: Depth");
    write_words(out, o);
    std::printf("PASS: polyeval host answers written\n");
    return 0;
}

static int evaluate(const char *in, const char *out) {
    const std::vector<uint64_t> w = read_words(in);
    size_t at = 0;
    const std::vector<uint64_t> hd = take(w, at, 7);
    const int logN = (int)hd[0], nq = (int)hd[1], np = (int)hd[2], beta = (int)hd[3], degree = (int)hd[4], B = (int)hd[6];
    const uint64_t t = hd[5];
    const size_t N = (size_t)1 << logN;
    const std::vector<uint64_t> q = take(w, at, (size_t)nq), p = take(w, at, (size_t)np);
    Context ctx(0);
    Ring ringQ(ctx, logN, q), ringP(ctx, logN, p);
    Evaluator eval(ringQ, ringP);
    const std::vector<uint64_t> kq = take(w, at, (size_t)beta * 2 * nq * N), kp = take(w, at, (size_t)beta * 2 * np * N);
    const EvaluationKey rlk = eval.NewEvaluationKey(beta, nq, np, kq, kp);
    const std::vector<polyeval::PowerInfo> held{{1, nq - 1, 1}};
    const polyeval::Plan plan(degree, HE_POLYEVAL_MONOMIAL, true, true, false, held, false);
    if (plan.leaves.size() != take(w, at, 1)[0]) throw std::runtime_error("polyeval_parity: another number of baby steps than the caller planned");
    size_t rows = 0;
    std::vector<int> ld, ll;
    for (const polyeval::LeafInfo &f : plan.leaves) { rows += (size_t)f.degree + 1; ld.push_back(f.degree); ll.push_back(f.level); }
    const std::vector<uint64_t> s0 = take(w, at, rows * nq), s1 = take(w, at, rows * nq);
    const polyeval::Polynomial pol(ringQ, degree, HE_POLYEVAL_MONOMIAL, true, true, false, held, ld, ll, s0, s1);
    Ciphertext ct{{ringQ.NewPoly(B), ringQ.NewPoly(B)}};
    for (Poly &v : ct.Value) v.Upload(take(w, at, (size_t)B * nq * N));
    Ciphertext res{{ringQ.AtLevel(plan.out_level).NewPoly(B), ringQ.AtLevel(plan.out_level).NewPoly(B)}};
    // the refusals arrive as exceptions before anything runs: no key where the plan relinearizes, an output that is the input
    int threw = 0;
    try { pol.Evaluate(eval, 1, t, nullptr, nq - 1, ct, {}, res); } catch (const Error &e) { threw += std::strstr(e.what(), "RelinearizationKey is nil") != nullptr; }
    try { Ciphertext bad{{ct.Value[0], res.Value[1]}}; pol.Evaluate(eval, 1, t, &rlk, nq - 1, ct, {}, bad); } catch (const Error &) { threw++; }
    if (threw != 2) throw std::runtime_error("polyeval_parity: a refusal did not arrive");
    pol.Evaluate(eval, 1, t, &rlk, nq - 1, ct, {}, res);
    // ... and the same through a basis of its own: EvaluateFromPowerBasis leaves the powers in it
    polyeval::PowerBasis pb(eval, HE_POLYEVAL_MONOMIAL, nq - 1, ct);
    Ciphertext res2{{ringQ.AtLevel(plan.out_level).NewPoly(B), ringQ.AtLevel(plan.out_level).NewPoly(B)}};
    pol.EvaluateFromPowerBasis(pb, 1, t, &rlk, {}, res2);
    if (pb.Powers().size() < 2) throw std::runtime_error("polyeval_parity: the basis holds no new power");
    ctx.Sync();
    std::vector<uint64_t> o;
    for (const Ciphertext *c : {&res, &res2})
        for (const Poly &v : c->Value) { const std::vector<uint64_t> d = v.Download(); o.insert(o.end(), d.begin(), d.end()); }
    write_words(out, o);
    std::printf("PASS: polyeval Evaluate results written\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--compile-only")) return 0;
    try {
        if (argc == 4 && !std::strcmp(argv[1], "--host")) return host(argv[2], argv[3]);
        if (argc == 4 && !std::strcmp(argv[1], "--evaluate")) return evaluate(argv[2], argv[3]);
        if (argc != 3) { std::fprintf(stderr, "usage: polyeval_parity [--host] IN OUT\n"); return 2; }
        const std::vector<uint64_t> w = read_words(argv[1]);
        size_t at = 0;
        const std::vector<uint64_t> hd = take(w, at, 5);
        const int logN = (int)hd[0], nq = (int)hd[1], degree = (int)hd[2], B = (int)hd[3], npowers = (int)hd[4];
        const size_t N = (size_t)1 << logN;
        const std::vector<uint64_t> q = take(w, at, (size_t)nq);
        Context ctx(0);
        Ring ringQ(ctx, logN, q);
        const std::vector<polyeval::PowerInfo> held{{1, nq - 1, 1}};
        const polyeval::Plan plan(degree, HE_POLYEVAL_MONOMIAL, true, true, false, held, false);
        if (plan.leaves.size() != take(w, at, 1)[0]) throw std::runtime_error("polyeval_parity: another number of baby steps than the caller planned");
        size_t rows = 0;
        std::vector<int> ld, ll;
        for (const polyeval::LeafInfo &f : plan.leaves) { rows += (size_t)f.degree + 1; ld.push_back(f.degree); ll.push_back(f.level); }
        const std::vector<uint64_t> s0 = take(w, at, rows * nq), s1 = take(w, at, rows * nq);
        polyeval::Polynomial pol(ringQ, degree, HE_POLYEVAL_MONOMIAL, true, true, false, held, ld, ll, s0, s1);
        std::vector<Ciphertext> X;
        for (int k = 0; k < npowers; k++) {
            X.push_back(Ciphertext{{ringQ.NewPoly(B), ringQ.NewPoly(B)}});
            for (Poly &v : X.back().Value) v.Upload(take(w, at, (size_t)B * nq * N));
        }
        std::vector<uint64_t> o;
        for (int G : {1, 4}) {
            pol.SetGroup(G);
            std::vector<Ciphertext> outs;
            for (const polyeval::LeafInfo &f : plan.leaves) outs.push_back(Ciphertext{{ringQ.AtLevel(f.level).NewPoly(B), ringQ.AtLevel(f.level).NewPoly(B)}});
            pol.EvaluatePolynomialFromPowerBasis(0, X, outs);
            ctx.Sync();
            for (const Ciphertext &c : outs)
                for (const Poly &v : c.Value) { const std::vector<uint64_t> d = v.Download(); o.insert(o.end(), d.begin(), d.end()); }
            if (G == 4) {  // a library rejection arrives as an exception: an output that is a power
                bool threw = false;
                try {
                    outs[0].Value[0] = X[0].Value[0];
                    pol.EvaluatePolynomialFromPowerBasis(0, X, outs);
                } catch (const Error &) { threw = true; }
                if (!threw) throw std::runtime_error("polyeval_parity: an output that is a power was accepted");
            }
        }
        write_words(argv[2], o);
        std::printf("PASS: polyeval mirror results written\n");
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
