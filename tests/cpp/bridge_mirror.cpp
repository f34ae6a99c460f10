// The CKKS bridge through the compiled mirror (include/hering.hpp): one RealToComplex -> ComplexToReal round trip and the two ring
// maps, on words read from a file and written to another (tests/test_cpp_bridge.py compares them with the Python mirror's).
//   bridge_mirror IN OUT        IN  (uint64 words): logN nq np beta | q[nq] | p[np] | stdToci q, p | ciToStd q, p | ct [2][nq][N/2]
//                               OUT (uint64 words): RealToComplex(ct) [2][nq][N] | ComplexToReal(that) [2][nq][N/2] |
//                                                   Unfold(ct[0]) [nq][N] | Fold(that) [nq][N/2]
//   bridge_mirror --compile-only   exits 0 (the header's new classes type-checked)
#include <cstdio>
#include <cstring>
#include <vector>

#include "hering.hpp"

using namespace hering;

static std::vector<uint64_t> take(const std::vector<uint64_t> &w, size_t &at, size_t n) {
    if (at + n > w.size()) throw std::runtime_error("bridge_mirror: input file too short");
    std::vector<uint64_t> v(w.begin() + at, w.begin() + at + n);
    at += n;
    return v;
}

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--compile-only")) return 0;
    if (argc != 3) { std::fprintf(stderr, "usage: bridge_mirror IN OUT\n"); return 2; }
    try {
        std::vector<uint64_t> w;
        {
            FILE *f = std::fopen(argv[1], "rb");
            if (!f) throw std::runtime_error("bridge_mirror: cannot open the input file");
            uint64_t buf[4096];
            size_t n;
            while ((n = std::fread(buf, 8, 4096, f)) > 0) w.insert(w.end(), buf, buf + n);
            std::fclose(f);
        }
        size_t at = 0;
        const std::vector<uint64_t> hd = take(w, at, 4);
        const int logN = (int)hd[0], nq = (int)hd[1], np = (int)hd[2], beta = (int)hd[3];
        const size_t N = (size_t)1 << logN, n = N / 2;
        const std::vector<uint64_t> q = take(w, at, nq), p = take(w, at, np);
        Context ctx(0);
        Ring ringQ(ctx, logN, q), ringP(ctx, logN, p), ringCI(ctx, logN - 1, q, RingType::ConjugateInvariant);
        Evaluator eval(ringQ, ringP);
        EvaluationKey keys[2];
        for (EvaluationKey &k : keys) {
            const std::vector<uint64_t> kq = take(w, at, (size_t)beta * 2 * nq * N), kp = take(w, at, (size_t)beta * 2 * np * N);
            k = eval.NewEvaluationKey(beta, nq, np, kq, kp);
        }
        ckks::DomainSwitcher sw(eval, keys[0], keys[1]);
        Ciphertext real{{ringCI.NewPoly(), ringCI.NewPoly()}}, cplx{{ringQ.NewPoly(), ringQ.NewPoly()}}, back{{ringCI.NewPoly(), ringCI.NewPoly()}};
        for (Poly &c : real.Value) c.Upload(take(w, at, (size_t)nq * n));
        sw.RealToComplex(real, cplx);
        sw.ComplexToReal(cplx, back);
        Poly un = ringQ.NewPoly(), fo = ringCI.NewPoly();
        ringQ.UnfoldConjugateInvariantToStandard(real.Value[0], un);
        ringCI.FoldStandardToConjugateInvariant(un, fo);
        ctx.Sync();
        FILE *f = std::fopen(argv[2], "wb");
        if (!f) throw std::runtime_error("bridge_mirror: cannot open the output file");
        for (const Poly *x : {&cplx.Value[0], &cplx.Value[1], &back.Value[0], &back.Value[1], &un, &fo}) {
            const std::vector<uint64_t> v = x->Download();
            std::fwrite(v.data(), 8, v.size(), f);
        }
        std::fclose(f);
        // the switcher without keys refuses, as the reference does
        bool threw = false;
        try { ckks::DomainSwitcher(eval, EvaluationKey(), EvaluationKey()).RealToComplex(real, cplx); } catch (const std::invalid_argument &) { threw = true; }
        if (!threw) throw std::runtime_error("bridge_mirror: a DomainSwitcher without keys did not refuse");
        std::printf("PASS: bridge mirror round trip written\n");
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
