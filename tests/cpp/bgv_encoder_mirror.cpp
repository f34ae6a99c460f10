// bgv.Encoder through the compiled mirror (include/hering.hpp, namespace bgv): IndexMatrix, EncodeRingT, DecodeRingT, RingT2Q,
// RingQ2T, Encode, EncodeQP and Decode on values read from a file, results written to another (tests/test_cpp_bgv_encoder.py
// compares them with the Python mirror's).
//   bgv_encoder_mirror IN OUT   IN  (uint64 words): logN logNT nq np batch T scale | q[nq] | p[np] | values [batch][N_T] (int64 bits)
//                               OUT (uint64 words): IndexMatrix | EncodeRingT -> [batch][N_T] | DecodeRingT of it [batch][N_T] |
//                                                   RingT2Q(scaleUp) -> [batch][nq][N] | RingQ2T(scaleDown) of it [batch][N_T] |
//                                                   Encode -> [batch][nq][N] | EncodeQP -> Q [batch][nq][N], P [batch][np][N] |
//                                                   Decode(Encode), int64 [batch][N_T]
//   bgv_encoder_mirror --compile-only   exits 0 (the header's new class type-checked)
#include <cstdio>
#include <cstring>
#include <vector>

#include "hering.hpp"

using namespace hering;

static std::vector<uint64_t> take(const std::vector<uint64_t> &w, size_t &at, size_t n) {
    if (at + n > w.size()) throw std::runtime_error("bgv_encoder_mirror: input file too short");
    std::vector<uint64_t> v(w.begin() + at, w.begin() + at + n);
    at += n;
    return v;
}
template <class T> static void put(FILE *f, const std::vector<T> &v) { std::fwrite(v.data(), 8, v.size(), f); }
static void put(FILE *f, const Poly &p) { put(f, p.Download()); }

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--compile-only")) return 0;
    if (argc != 3) { std::fprintf(stderr, "usage: bgv_encoder_mirror IN OUT\n"); return 2; }
    try {
        std::vector<uint64_t> w;
        {
            FILE *f = std::fopen(argv[1], "rb");
            if (!f) throw std::runtime_error("bgv_encoder_mirror: cannot open the input file");
            uint64_t buf[4096];
            size_t n;
            while ((n = std::fread(buf, 8, 4096, f)) > 0) w.insert(w.end(), buf, buf + n);
            std::fclose(f);
        }
        size_t at = 0;
        const std::vector<uint64_t> hd = take(w, at, 7);
        const int logN = (int)hd[0], logNT = (int)hd[1], nq = (int)hd[2], np = (int)hd[3], batch = (int)hd[4];
        const uint64_t T = hd[5], scale = hd[6];
        const std::vector<uint64_t> q = take(w, at, nq), p = take(w, at, np);
        const std::vector<uint64_t> bits = take(w, at, (size_t)batch << logNT);
        std::vector<int64_t> values(bits.size());
        std::memcpy(values.data(), bits.data(), bits.size() * 8);

        Context ctx(0);
        Ring ringQ(ctx, logN, q), ringP(ctx, logN, p), ringT(ctx, logNT, {T});
        bgv::Encoder enc(ringQ, ringT, &ringP);
        if (enc.LogMaxSlots() != logNT || enc.LogGap() != logN - logNT || enc.RingQ2TMaxLimbs() != 32) throw std::runtime_error("bgv_encoder_mirror: info");
        bgv::MetaData m;
        m.Scale = scale; m.IsNTT = true; m.IsMontgomery = false;

        FILE *f = std::fopen(argv[2], "wb");
        if (!f) throw std::runtime_error("bgv_encoder_mirror: cannot open the output file");
        put(f, enc.IndexMatrix());
        Poly pT = ringT.NewPoly(batch), back = ringT.NewPoly(batch);
        enc.EncodeRingT(values, scale, pT);
        put(f, pT);
        std::vector<uint64_t> words;
        enc.DecodeRingT(pT, scale, words);
        put(f, words);
        Poly pt = ringQ.NewPoly(batch), pq = ringQ.NewPoly(batch), pp = ringP.NewPoly(batch);
        enc.RingT2Q(pt.Level(), true, pT, pt);
        put(f, pt);
        enc.RingQ2T(pt.Level(), true, pt, back);
        put(f, back);
        enc.Encode(values, m, pt);
        put(f, pt);
        bgv::MetaData mqp = m;
        mqp.IsMontgomery = true;
        enc.EncodeQP(values, false, mqp, pq, pp);
        put(f, pq);
        put(f, pp);
        std::vector<int64_t> dec;
        enc.Decode(pt, m, dec);
        put(f, dec);
        std::fclose(f);
        // a library rejection arrives as an exception
        bool threw = false;
        m.Scale = 0;
        try { enc.Encode(values, m, pt); } catch (const Error &e) { threw = e.code == HE_EINVAL; }
        if (!threw) throw std::runtime_error("bgv_encoder_mirror: the scale 0 was accepted");
        std::printf("PASS: bgv encoder mirror results written\n");
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
