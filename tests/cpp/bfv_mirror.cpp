// BFV through the compiled mirror (include/hering.hpp, namespace bgv): one MulRelinScaleInvariant, one MulScaleInvariant, the
// squaring call and one Quantize, on words read from a file and written to another (tests/test_cpp_bfv.py compares them with the
// Python mirror's).
//   bfv_mirror IN OUT        IN  (uint64 words): logN nq np nm beta t | q[nq] | p[np] | qmul[nm] | rlk q, p | ct0 [2][nq][N] |
//                                                ct1 [2][nq][N] | cM [nm][N]
//                            OUT (uint64 words): MulRelinScaleInvariant(ct0, ct1) [2][nq][N] | MulScaleInvariant(ct0, ct1) [3][nq][N] |
//                                                MulRelinScaleInvariant(ct0, ct0) [2][nq][N] | Quantize(ct1[0], cM) [nq][N]
//   bfv_mirror --compile-only   exits 0 (the header's new class type-checked)
#include <cstdio>
#include <cstring>
#include <vector>

#include "hering.hpp"

using namespace hering;

static std::vector<uint64_t> take(const std::vector<uint64_t> &w, size_t &at, size_t n) {
    if (at + n > w.size()) throw std::runtime_error("bfv_mirror: input file too short");
    std::vector<uint64_t> v(w.begin() + at, w.begin() + at + n);
    at += n;
    return v;
}

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--compile-only")) return 0;
    if (argc != 3) { std::fprintf(stderr, "usage: bfv_mirror IN OUT\n"); return 2; }
    try {
        std::vector<uint64_t> w;
        {
            FILE *f = std::fopen(argv[1], "rb");
            if (!f) throw std::runtime_error("bfv_mirror: cannot open the input file");
            uint64_t buf[4096];
            size_t n;
            while ((n = std::fread(buf, 8, 4096, f)) > 0) w.insert(w.end(), buf, buf + n);
            std::fclose(f);
        }
        size_t at = 0;
        const std::vector<uint64_t> hd = take(w, at, 6);
        const int logN = (int)hd[0], nq = (int)hd[1], np = (int)hd[2], nm = (int)hd[3], beta = (int)hd[4];
        const uint64_t t = hd[5];
        const size_t N = (size_t)1 << logN;
        const std::vector<uint64_t> q = take(w, at, nq), p = take(w, at, np), qm = take(w, at, nm);
        Context ctx(0);
        Ring ringQ(ctx, logN, q), ringP(ctx, logN, p), ringQMul(ctx, logN, qm);
        Evaluator eval(ringQ, ringP);
        const std::vector<uint64_t> kq = take(w, at, (size_t)beta * 2 * nq * N), kp = take(w, at, (size_t)beta * 2 * np * N);
        const EvaluationKey rlk = eval.NewEvaluationKey(beta, nq, np, kq, kp);
        bgv::Evaluator bfv(eval, ringQMul, t, rlk);
        if ((int)bfv.LevelQMul().size() != nq || bfv.LevelQMul().back() != nm - 1) throw std::runtime_error("bfv_mirror: levelQMul");
        Ciphertext ct0{{ringQ.NewPoly(), ringQ.NewPoly()}}, ct1{{ringQ.NewPoly(), ringQ.NewPoly()}};
        for (Ciphertext *c : {&ct0, &ct1})
            for (Poly &v : c->Value) v.Upload(take(w, at, (size_t)nq * N));
        Poly cM = ringQMul.NewPoly();
        cM.Upload(take(w, at, (size_t)nm * N));
        Ciphertext relin{{ringQ.NewPoly(), ringQ.NewPoly()}}, deg2{{ringQ.NewPoly(), ringQ.NewPoly(), ringQ.NewPoly()}};
        Ciphertext sq{{ringQ.NewPoly(), ringQ.NewPoly()}};
        bfv.MulRelinScaleInvariant(ct0, ct1, relin);
        bfv.MulScaleInvariant(ct0, ct1, deg2);
        bfv.MulRelinScaleInvariant(ct0, ct0, sq);
        bfv.Quantize(nq - 1, ct1.Value[0], cM);  // (in place, as the reference: after the products that read ct1)
        ctx.Sync();
        FILE *f = std::fopen(argv[2], "wb");
        if (!f) throw std::runtime_error("bfv_mirror: cannot open the output file");
        for (const Poly *x : {&relin.Value[0], &relin.Value[1], &deg2.Value[0], &deg2.Value[1], &deg2.Value[2], &sq.Value[0], &sq.Value[1], &ct1.Value[0]}) {
            const std::vector<uint64_t> v = x->Download();
            std::fwrite(v.data(), 8, v.size(), f);
        }
        std::fclose(f);
        // without a key the evaluator refuses to relinearise, and a library rejection arrives as an exception
        bool threw = false;
        try { bgv::Evaluator(eval, ringQMul, t).MulRelinScaleInvariant(ct0, ct1, relin); } catch (const std::invalid_argument &) { threw = true; }
        if (!threw) throw std::runtime_error("bfv_mirror: an evaluator without a key did not refuse");
        threw = false;
        try { bgv::Evaluator(eval, ringP, t); } catch (const Error &) { threw = true; }  // (too few moduli for the top level)
        if (!threw) throw std::runtime_error("bfv_mirror: a short ringQMul was accepted");
        std::printf("PASS: bfv mirror results written\n");
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
