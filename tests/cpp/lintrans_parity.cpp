// Linear transformations through the compiled mirror (include/hering.hpp, namespace lintrans): one BSGS and one naive
// transformation in one EvaluateMany, then EvaluateSequential of the two, on words read from a file and written to another
// (tests/test_cpp_lintrans.py compares them with the oracle's).
//   lintrans_parity IN OUT   IN  (uint64 words): logN nq np beta log_slots nkeys | q[nq] | p[np] |
//                                                per key: galEl, q words [beta][2][nq][N], p words [beta][2][np][N] |
//                                                2 transformations: N1 ndiag | per diagonal: index, Q [nq][N], P [np][N] |
//                                                ct [2][nq][N]
//                            OUT (uint64 words): EvaluateMany -> out_a [2][nq][N], out_b [2][nq][N] | EvaluateSequential(a, b) [2][nq][N]
//   lintrans_parity --compile-only   exits 0 (the header's new namespace type-checked)
#include <cstdio>
#include <cstring>
#include <vector>

#include "hering.hpp"

using namespace hering;

static std::vector<uint64_t> take(const std::vector<uint64_t> &w, size_t &at, size_t n) {
    if (at + n > w.size()) throw std::runtime_error("lintrans_parity: input file too short");
    std::vector<uint64_t> v(w.begin() + at, w.begin() + at + n);
    at += n;
    return v;
}

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--compile-only")) return 0;
    if (argc != 3) { std::fprintf(stderr, "usage: lintrans_parity IN OUT\n"); return 2; }
    try {
        std::vector<uint64_t> w;
        {
            FILE *f = std::fopen(argv[1], "rb");
            if (!f) throw std::runtime_error("lintrans_parity: cannot open the input file");
            uint64_t buf[4096];
            size_t n;
            while ((n = std::fread(buf, 8, 4096, f)) > 0) w.insert(w.end(), buf, buf + n);
            std::fclose(f);
        }
        size_t at = 0;
        const std::vector<uint64_t> hd = take(w, at, 6);
        const int logN = (int)hd[0], nq = (int)hd[1], np = (int)hd[2], beta = (int)hd[3], logSlots = (int)hd[4], nkeys = (int)hd[5];
        const size_t N = (size_t)1 << logN;
        const std::vector<uint64_t> q = take(w, at, nq), p = take(w, at, np);
        Context ctx(0);
        Ring ringQ(ctx, logN, q), ringP(ctx, logN, p);
        Evaluator eval(ringQ, ringP);
        std::vector<uint64_t> galEls;
        std::vector<EvaluationKey> keys;
        for (int k = 0; k < nkeys; k++) {
            galEls.push_back(take(w, at, 1)[0]);
            const std::vector<uint64_t> kq = take(w, at, (size_t)beta * 2 * nq * N), kp = take(w, at, (size_t)beta * 2 * np * N);
            keys.push_back(eval.NewEvaluationKey(beta, nq, np, kq, kp));
        }
        blindrot::GaloisKeySet gks(eval, galEls, keys);
        std::vector<lintrans::LinearTransformation> lts;
        std::vector<std::vector<int>> diags;
        for (int t = 0; t < 2; t++) {
            const std::vector<uint64_t> h = take(w, at, 2);
            std::vector<int> idx;
            std::vector<Poly> Q, P;
            for (uint64_t d = 0; d < h[1]; d++) {
                idx.push_back((int)(int64_t)take(w, at, 1)[0]);
                Q.push_back(ringQ.NewPoly());
                Q.back().Upload(take(w, at, (size_t)nq * N));
                P.push_back(ringP.NewPoly());
                P.back().Upload(take(w, at, (size_t)np * N));
            }
            lts.emplace_back(eval, nq - 1, np - 1, logSlots, (int)h[0], idx, Q, P);
            diags.push_back(idx);
        }
        // the index entries through the mirror: the Galois elements the key set was made for cover what the transformations ask for
        for (int t = 0; t < 2; t++) {
            const int N1 = lts[(size_t)t].N1;
            if (N1 != 0 && lintrans::BSGSIndex(diags[(size_t)t], 1 << logSlots, N1).first.empty()) throw std::runtime_error("lintrans_parity: BSGSIndex");
        }
        if (lintrans::FindBestBSGSRatio({0, 1, 2, 3}, 64, 0) != 2) throw std::runtime_error("lintrans_parity: FindBestBSGSRatio");
        if (lintrans::GaloisElements(eval, {0, 1, 2, 3}, 1 << logSlots, -1).size() != 4) throw std::runtime_error("lintrans_parity: GaloisElements");
        Ciphertext ct{{ringQ.NewPoly(), ringQ.NewPoly()}};
        for (Poly &v : ct.Value) v.Upload(take(w, at, (size_t)nq * N));
        std::vector<Ciphertext> outs;
        for (int t = 0; t < 2; t++) outs.push_back(Ciphertext{{ringQ.NewPoly(), ringQ.NewPoly()}});
        Ciphertext seq{{ringQ.NewPoly(), ringQ.NewPoly()}};
        lintrans::Evaluator lev(eval, gks);
        lts[0].SetGroup(2);
        lev.EvaluateMany(nq - 1, ct, lts, outs);
        lev.EvaluateSequential(nq - 1, ct, lts, seq);
        ctx.Sync();
        FILE *f = std::fopen(argv[2], "wb");
        if (!f) throw std::runtime_error("lintrans_parity: cannot open the output file");
        for (const Poly *x : {&outs[0].Value[0], &outs[0].Value[1], &outs[1].Value[0], &outs[1].Value[1], &seq.Value[0], &seq.Value[1]}) {
            const std::vector<uint64_t> v = x->Download();
            std::fwrite(v.data(), 8, v.size(), f);
        }
        std::fclose(f);
        // a library rejection arrives as an exception: two outputs that are one polynomial
        bool threw = false;
        try {
            Ciphertext bad{{outs[0].Value[0], outs[0].Value[0]}};
            lev.Evaluate(nq - 1, ct, lts[0], bad);
        } catch (const Error &) { threw = true; }
        if (!threw) throw std::runtime_error("lintrans_parity: one polynomial for both outputs was accepted");
        std::printf("PASS: lintrans mirror results written\n");
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
