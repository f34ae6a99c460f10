// The ring samplers through the compiled mirror (include/hering.hpp): UniformSampler (ring and ringqp forms), GaussianSampler and
// TernarySampler over a PRNG that serves the bytes of a file, results and positions written to another
// (tests/test_cpp_sampler.py compares them with the Python mirror's on the same bytes).
//   sampler_mirror IN OUT   IN  (uint64 words): logN nq np batch nbytes | q[nq] | p[np] | the stream, nbytes bytes padded to words
//                           OUT (uint64 words): uniform Q, P | position | Gaussian (sigma 3.2, bound 19.2, Montgomery) | position |
//                                               ternary (P = 2/3) added to the Gaussian | position | ternary (P = 0.5) | position
//   sampler_mirror --compile-only   exits 0 (the header's new classes type-checked)
#include <cstdio>
#include <cstring>
#include <vector>

#include "hering.hpp"

using namespace hering;

static std::vector<uint64_t> take(const std::vector<uint64_t> &w, size_t &at, size_t n) {
    if (at + n > w.size()) throw std::runtime_error("sampler_mirror: input file too short");
    std::vector<uint64_t> v(w.begin() + at, w.begin() + at + n);
    at += n;
    return v;
}
static void put(FILE *f, const std::vector<uint64_t> &v) { std::fwrite(v.data(), 8, v.size(), f); }
static void put(FILE *f, const Poly &p) { put(f, p.Download()); }
static void put(FILE *f, uint64_t v) { std::fwrite(&v, 8, 1, f); }

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--compile-only")) return 0;
    if (argc != 3) { std::fprintf(stderr, "usage: sampler_mirror IN OUT\n"); return 2; }
    try {
        std::vector<uint64_t> w;
        {
            FILE *f = std::fopen(argv[1], "rb");
            if (!f) throw std::runtime_error("sampler_mirror: cannot open the input file");
            uint64_t buf[4096];
            size_t n;
            while ((n = std::fread(buf, 8, 4096, f)) > 0) w.insert(w.end(), buf, buf + n);
            std::fclose(f);
        }
        size_t at = 0;
        const std::vector<uint64_t> hd = take(w, at, 5);
        const int logN = (int)hd[0], nq = (int)hd[1], np = (int)hd[2], batch = (int)hd[3];
        const size_t nbytes = (size_t)hd[4];
        const std::vector<uint64_t> q = take(w, at, nq), p = take(w, at, np);
        const std::vector<uint64_t> stream = take(w, at, (nbytes + 7) / 8);
        size_t served = 0;
        sampling::PRNG prng([&](uint8_t *dst, size_t n) {
            if (served + n > nbytes) return false;
            std::memcpy(dst, reinterpret_cast<const uint8_t *>(stream.data()) + served, n);
            served += n;
            return true;
        });

        Context ctx(0);
        Ring ringQ(ctx, logN, q), ringP(ctx, logN, p);
        FILE *f = std::fopen(argv[2], "wb");
        if (!f) throw std::runtime_error("sampler_mirror: cannot open the output file");
        Poly uq = ringQ.NewPoly(batch), up = ringP.NewPoly(batch);
        UniformSampler(prng, ringQ, ringP).Read(uq, up);
        put(f, uq);
        put(f, up);
        put(f, prng.Position());
        Poly e = GaussianSampler(prng, ringQ, DiscreteGaussian{3.2, 19.2}, true).ReadNew(batch);
        put(f, e);
        put(f, prng.Position());
        TernarySampler(prng, ringQ, Ternary{2.0 / 3.0}, true).ReadAndAdd(e);
        put(f, e);
        put(f, prng.Position());
        put(f, TernarySampler(prng, ringQ.AtLevel(0), Ternary{0.5}, false).ReadNew(batch));
        put(f, prng.Position());
        std::fclose(f);
        // a library rejection arrives as an exception: a source that runs short
        bool threw = false;
        served = nbytes;
        try {
            for (int i = 0; i < 64; i++) UniformSampler(prng, ringQ).ReadNew(batch);
        } catch (const Error &err) { threw = err.code == HE_EPRNG; }
        if (!threw) throw std::runtime_error("sampler_mirror: the exhausted source was accepted");
        std::printf("PASS: sampler mirror results written\n");
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
