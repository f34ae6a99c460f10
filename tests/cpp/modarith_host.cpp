// The integer primitives of lattigo_amd/csrc/modarith.h as a plain host program (g++, no library, no device): tests/test_arith_host.py
// feeds it the operand sets of tests/arith_ref.py and compares every word with the same references the device is held against.
//
// stdin, binary, any number of jobs: eight words {magic, op, q, qinv, brc0, brc1, n, 0}, then a[n] and b[n] (b is sent for every
// op; one-operand ops ignore it).  stdout: out[n] per job.  op: the HE_ARITH_* numbering of include/hering_debug.h, MRED_LAZY ..
// IMFORM without the hand-written form, which exists on the device only; 13 (here only): mred_w32, the canonical form of op 2.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "modarith.h"

namespace {
constexpr uint64_t kMagic = 0x4152495448303031ull;  // "ARITH001"
bool read_words(uint64_t *p, size_t n) { return fread(p, 8, n, stdin) == n; }
}  // namespace

int main() {
    uint64_t h[8];
    std::vector<uint64_t> a, b, o;
    while (read_words(h, 8)) {
        const uint64_t op = h[1], q = h[2], qinv = h[3], brc0 = h[4], brc1 = h[5];
        const size_t n = (size_t)h[6];
        if (h[0] != kMagic || n == 0 || n > ((size_t)1 << 20)) { fprintf(stderr, "modarith_host: bad job header\n"); return 2; }
        a.resize(n); b.resize(n); o.resize(n);
        if (!read_words(a.data(), n) || !read_words(b.data(), n)) { fprintf(stderr, "modarith_host: short job\n"); return 2; }
        for (size_t i = 0; i < n; i++) {
            const uint64_t x = a[i], y = b[i];
            switch (op) {
            case 0: o[i] = he::mred_lazy(x, y, q, qinv); break;
            case 1: o[i] = he::mred(x, y, q, qinv); break;
            case 2: o[i] = he::mred_lazy_w32(x, y, q, qinv); break;
            case 4: o[i] = he::mred128_lazy(x, y, q, qinv); break;
            case 5: o[i] = he::bred_add_lazy(x, q, brc0); break;
            case 6: o[i] = he::bred_add(x, q, brc0); break;
            case 7: o[i] = he::bred_lazy(x, y, q, brc0, brc1); break;
            case 8: o[i] = he::bred(x, y, q, brc0, brc1); break;
            case 9: o[i] = he::mform_lazy(x, q, brc0, brc1); break;
            case 10: o[i] = he::mform(x, q, brc0, brc1); break;
            case 11: o[i] = he::imform_lazy(x, q, qinv); break;
            case 12: o[i] = he::imform(x, q, qinv); break;
            case 13: o[i] = he::mred_w32(x, y, q, qinv); break;  // (canonical form of op 2: equals op 1)
            default: fprintf(stderr, "modarith_host: unknown op %llu\n", (unsigned long long)op); return 2;
            }
        }
        if (fwrite(o.data(), 8, n, stdout) != n) return 3;
    }
    return fflush(stdout) == 0 ? 0 : 3;
}
