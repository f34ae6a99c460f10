// rlwe.Encryptor / rlwe.Decryptor / KeyGenerator.GenPublicKey through the compiled mirror (include/hering.hpp, namespace rlwe): one
// BGV vector encoded, encrypted under sk and under the pk that GenPublicKey made, decrypted and decoded, all on the device, from the
// system source.
//   encryptor_mirror                  prints PASS and exits 0 when both round trips return the values
//   encryptor_mirror --compile-only   exits 0 (the header's new classes type-checked)
#include <cstdio>
#include <cstring>
#include <vector>

#include "hering.hpp"

using namespace hering;

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "--compile-only")) return 0;
    try {
        const int logN = 10, N = 1 << logN;
        const uint64_t T = 65537;
        const std::vector<uint64_t> q = {0x1fffffffffe00001ull, 0x1fffffffffc80001ull, 0x1fffffffffb40001ull}, p = {0x1ffffffff6c80001ull, 0x1ffffffff6140001ull};
        Context ctx(0);
        Ring ringQ(ctx, logN, q), ringP(ctx, logN, p), ringT(ctx, logN, {T});
        Evaluator eval(ringQ, ringP);
        sampling::PRNG prng;

        // a ternary secret of density 2/3 from the source, brought to the NTT domain and Montgomery form as the reference holds it
        rlwe::SecretKey sk{{ringQ.NewPoly(), ringP.NewPoly()}};
        TernarySampler(prng, ringQ, Ternary{}, false).Read(sk.Value.Q);
        check(he_centered_lift(eval.h(), 3, sk.Value.Q.h(), ringQ.Level() + 1, ringQ.Level(), sk.Value.Q.h(), ringP.Level(), sk.Value.P.h()));
        ringQ.NTT(sk.Value.Q, sk.Value.Q);
        ringQ.MForm(sk.Value.Q, sk.Value.Q);
        ringP.NTT(sk.Value.P, sk.Value.P);
        ringP.MForm(sk.Value.P, sk.Value.P);

        rlwe::PublicKey pk{{{{ringQ.NewPoly(), ringP.NewPoly()}, {ringQ.NewPoly(), ringP.NewPoly()}}}};
        rlwe::KeyGenerator(eval, prng).GenPublicKey(sk, pk);

        bgv::Encoder ecd(ringQ, ringT, &ringP);
        std::vector<uint64_t> values((size_t)N);
        for (int i = 0; i < N; i++) values[i] = (uint64_t)(i * 7919 + 3) % T;
        rlwe::Plaintext pt{ringQ.NewPoly(), {true, false}};
        ecd.Encode(values, bgv::MetaData{}, pt.Value);

        rlwe::Encryptor enc(eval, prng);
        rlwe::Decryptor dec(eval, sk);
        const rlwe::Encryptor encs[2] = {enc.WithKey(sk), enc.WithKey(pk)};
        for (int k = 0; k < 2; k++) {
            rlwe::Ciphertext ct{{ringQ.NewPoly(), ringQ.NewPoly()}, {}};
            encs[k].Encrypt(pt, ct);
            if (ct.Value[0].Download() == pt.Value.Download()) throw std::runtime_error("the ciphertext is the plaintext");
            rlwe::Plaintext out{ringQ.NewPoly(), {}};
            dec.Decrypt(ct, out);
            std::vector<uint64_t> got;
            ecd.Decode(out.Value, bgv::MetaData{}, got);
            if (got != values) throw std::runtime_error(k ? "pk round trip: values differ" : "sk round trip: values differ");
        }
        if (prng.Position() == 0) throw std::runtime_error("the source was not read");
        std::printf("PASS: BGV round trip under sk and pk\n");
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "FAIL: %s\n", e.what());
        return 1;
    }
}
