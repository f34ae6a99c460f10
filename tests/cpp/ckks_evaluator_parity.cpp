// The compiled mirror ckks::Evaluator (include/hering.hpp) over the four entries of include/hering_ckks_evaluator.h, each run once on
// words read from a file; the results are written to another (tests/test_cpp_ckks_evaluator.py compares them with known answers
// made from tests/ckks_evaluator_ref.py over the oracle's ring primitives).
//   ckks_evaluator_parity --compile-only   exits 0 (the header's namespace type-checked and linked)
//   ckks_evaluator_parity IN OUT           IN: logN nq np beta B | q[nq] | p[np] | key q words [beta][2][nq][N], p words [beta][2][np][N] |
//                                              ratio[nq] s0[nq] s1[nq] pre[nq] | a [2][B][nq][N] | b [3][B][nq][N] | pt [1][nq][N] |
//                                              acc [3][B][nq][N]
//                                          OUT: AddSub(sub, scaled 2) [3] | Scalar(MUL_THEN_ADD, pre) onto acc [2] | MulPlaintext [2] |
//                                               MulPlaintext(thenAdd, pre) onto acc [2] | MulRelinThenAdd without a key onto acc [3] |
//                                               MulRelinThenAdd with the key and pre onto acc [2]; every component [B][nq][N]
#include <cstdio>
#include <cstring>
#include <vector>

#include "hering.hpp"

using namespace hering;

static std::vector<uint64_t> read_words(const char *path) {
    std::vector<uint64_t> w;
    FILE *f = std::fopen(path, "rb");
    if (!f) throw std::runtime_error("ckks_evaluator_parity: cannot open the input file");
    uint64_t buf[4096];
    size_t n;
    while ((n = std::fread(buf, 8, 4096, f)) > 0) w.insert(w.end(), buf, buf + n);
    std::fclose(f);
    return w;
}
static std::vector<uint64_t> take(const std::vector<uint64_t> &w, size_t &at, size_t n) {
    if (at + n > w.size()) throw std::runtime_error("ckks_evaluator_parity: input file too short");
    std::vector<uint64_t> v(w.begin() + at, w.begin() + at + n);
    at += n;
    return v;
}

static int run(const char *in, const char *out) {
    const std::vector<uint64_t> w = read_words(in);
    size_t at = 0;
    const std::vector<uint64_t> hd = take(w, at, 5);
    const int logN = (int)hd[0], nq = (int)hd[1], np = (int)hd[2], beta = (int)hd[3], B = (int)hd[4], level = nq - 1;
    const size_t N = (size_t)1 << logN;
    const std::vector<uint64_t> q = take(w, at, (size_t)nq), p = take(w, at, (size_t)np);
    Context ctx(0);
    Ring ringQ(ctx, logN, q), ringP(ctx, logN, p);
    Evaluator eval(ringQ, ringP);
    const std::vector<uint64_t> kq = take(w, at, (size_t)beta * 2 * nq * N), kp = take(w, at, (size_t)beta * 2 * np * N);
    const EvaluationKey rlk = eval.NewEvaluationKey(beta, nq, np, kq, kp);
    const std::vector<uint64_t> ratio = take(w, at, (size_t)nq), s0 = take(w, at, (size_t)nq), s1 = take(w, at, (size_t)nq), pre = take(w, at, (size_t)nq);
    auto load = [&](int n, int batch) {
        Ciphertext c;
        for (int i = 0; i < n; i++) {
            c.Value.push_back(ringQ.NewPoly(batch));
            c.Value.back().Upload(take(w, at, (size_t)batch * nq * N));
        }
        return c;
    };
    const Ciphertext a = load(2, B), b = load(3, B), pt = load(1, 1);
    const size_t acc_at = at;
    auto acc = [&](int n) { at = acc_at; return load(n, B); };
    const ckks::Evaluator ev(ringQ, &eval);
    std::vector<uint64_t> o;
    auto emit = [&](const Ciphertext &c) {
        ctx.Sync();
        for (const Poly &v : c.Value) { const std::vector<uint64_t> d = v.Download(); o.insert(o.end(), d.begin(), d.end()); }
    };
    {
        Ciphertext r{{ringQ.NewPoly(B), ringQ.NewPoly(B), ringQ.NewPoly(B)}};
        ev.AddSub(level, true, a, b, 2, &ratio, r);
        emit(r);
    }
    { Ciphertext r = acc(2); ev.Scalar(level, HE_CKKS_SCALAR_MUL_THEN_ADD, a, s0, s1, &pre, r); emit(r); }
    { Ciphertext r{{ringQ.NewPoly(B), ringQ.NewPoly(B)}}; ev.MulPlaintext(level, a, pt.Value[0], false, nullptr, r); emit(r); }
    { Ciphertext r = acc(2); ev.MulPlaintext(level, a, pt.Value[0], true, &pre, r); emit(r); }
    const Ciphertext b2{{b.Value[0], b.Value[1]}};
    { Ciphertext r = acc(3); ev.MulRelinThenAdd(level, a, b2, nullptr, nullptr, r); emit(r); }
    {
        Ciphertext r = acc(2);
        int threw = 0;  // an output that is an input is refused before anything runs
        try { Ciphertext bad{{a.Value[0], r.Value[1]}}; ev.MulRelinThenAdd(level, a, b2, &rlk, nullptr, bad); } catch (const Error &) { threw++; }
        if (threw != 1) throw std::runtime_error("ckks_evaluator_parity: a refusal did not arrive");
        ev.MulRelinThenAdd(level, a, b2, &rlk, &pre, r);
        emit(r);
    }
    FILE *f = std::fopen(out, "wb");
    if (!f) throw std::runtime_error("ckks_evaluator_parity: cannot open the output file");
    std::fwrite(o.data(), 8, o.size(), f);
    std::fclose(f);
    std::printf("PASS: ckks evaluator results written\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--compile-only")) return 0;
    try {
        if (argc != 3) { std::fprintf(stderr, "usage: ckks_evaluator_parity [--compile-only | IN OUT]\n"); return 2; }
        return run(argv[1], argv[2]);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "FAIL: %s\n", e.what());
        return 1;
    }
}
