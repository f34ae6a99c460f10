// ckks.Encoder through the compiled mirror (include/hering.hpp, namespace ckks): FFT, IFFT, Encode, EncodeQP and Decode on values
// read from a file, results written to another (tests/test_cpp_ckks_encoder.py compares them with the Python mirror's).
//   ckks_encoder_mirror IN OUT   IN  (uint64 words): logN nq np logSlots batch scale(bits) | q[nq] | p[np] | values [batch][slots][2] (bits)
//                                OUT (uint64 words): FFT(values) | IFFT(values) (float64 bits) | Encode -> [batch][nq][N] |
//                                                    EncodeQP -> Q [batch][nq][N], P [batch][np][N] | Decode(Encode) [batch][slots][2] (bits)
//   ckks_encoder_mirror --compile-only   exits 0 (the header's new class type-checked)
#include <cstdio>
#include <cstring>
#include <vector>

#include "hering.hpp"

using namespace hering;

static std::vector<uint64_t> take(const std::vector<uint64_t> &w, size_t &at, size_t n) {
    if (at + n > w.size()) throw std::runtime_error("ckks_encoder_mirror: input file too short");
    std::vector<uint64_t> v(w.begin() + at, w.begin() + at + n);
    at += n;
    return v;
}
static void put(FILE *f, const std::vector<std::complex<double>> &v) { std::fwrite(v.data(), 16, v.size(), f); }
static void put(FILE *f, const Poly &p) {
    const std::vector<uint64_t> v = p.Download();
    std::fwrite(v.data(), 8, v.size(), f);
}

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--compile-only")) return 0;
    if (argc != 3) { std::fprintf(stderr, "usage: ckks_encoder_mirror IN OUT\n"); return 2; }
    try {
        std::vector<uint64_t> w;
        {
            FILE *f = std::fopen(argv[1], "rb");
            if (!f) throw std::runtime_error("ckks_encoder_mirror: cannot open the input file");
            uint64_t buf[4096];
            size_t n;
            while ((n = std::fread(buf, 8, 4096, f)) > 0) w.insert(w.end(), buf, buf + n);
            std::fclose(f);
        }
        size_t at = 0;
        const std::vector<uint64_t> hd = take(w, at, 6);
        const int logN = (int)hd[0], nq = (int)hd[1], np = (int)hd[2], logSlots = (int)hd[3], batch = (int)hd[4];
        double scale;
        std::memcpy(&scale, &hd[5], 8);
        const std::vector<uint64_t> q = take(w, at, nq), p = take(w, at, np);
        const size_t slots = (size_t)1 << logSlots;
        const std::vector<uint64_t> bits = take(w, at, (size_t)batch * slots * 2);
        std::vector<std::complex<double>> values((size_t)batch * slots);
        std::memcpy(static_cast<void *>(values.data()), bits.data(), bits.size() * 8);

        Context ctx(0);
        Ring ringQ(ctx, logN, q), ringP(ctx, logN, p);
        ckks::Encoder enc(ringQ, &ringP);
        if (enc.LogMaxSlots() != logN - 1 || enc.Roots().size() != ((size_t)2 << logN) + 1) throw std::runtime_error("ckks_encoder_mirror: info");
        if (enc.Roots() != ckks::Encoder::RootsHost((uint64_t)2 << logN)) throw std::runtime_error("ckks_encoder_mirror: the built-in table");
        ckks::MetaData m;
        m.Scale = scale; m.LogSlots = logSlots; m.IsNTT = true; m.IsMontgomery = false;

        FILE *f = std::fopen(argv[2], "wb");
        if (!f) throw std::runtime_error("ckks_encoder_mirror: cannot open the output file");
        std::vector<std::complex<double>> v = values;
        enc.FFT(v, logSlots);
        put(f, v);
        v = values;
        enc.IFFT(v, logSlots);
        put(f, v);
        Poly pt = ringQ.NewPoly(batch), pq = ringQ.NewPoly(batch), pp = ringP.NewPoly(batch);
        enc.Encode(values, m, pt);
        put(f, pt);
        ckks::MetaData mqp = m;
        mqp.IsMontgomery = true;
        enc.EncodeQP(values, mqp, pq, pp);
        put(f, pq);
        put(f, pp);
        put(f, enc.Decode(pt, m));
        std::fclose(f);
        // a library rejection arrives as an exception
        bool threw = false;
        m.LogSlots = logN;
        try { enc.Encode(values, m, pt); } catch (const Error &e) { threw = e.code == HE_EINVAL; }
        if (!threw) throw std::runtime_error("ckks_encoder_mirror: logSlots above the maximum was accepted");
        std::printf("PASS: ckks encoder mirror results written\n");
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
