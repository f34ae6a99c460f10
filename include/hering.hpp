// hering.hpp -- header-only C++17 host side of libhering.so (include/hering.h).
//
// The reference's host code is compiled (Go); this image has no Go toolchain, so beside the cgo package under go/hering (shipped
// as source) this header is the COMPILED mirror of the reference's operator interfaces for the hot path: the same type and method
// names, argument order (outputs last, caller-allocated) and error behaviour as
//     ring.Ring                    ring/ring.go, ring/ntt.go:127-152, ring/operations.go, ring/scaling.go, ring/automorphism.go
//     ring.BasisExtender           ring/basis_extension.go:14-280
//     rlwe.Evaluator               core/rlwe/evaluator*.go   (the seven EvaluatorProvider methods of core/rlwe/rlwe.go:10-18 included)
//     ckks / bgv Evaluator         MulRelin (schemes/ckks/evaluator.go:764, schemes/bgv/evaluator.go:592), Rescale (:477 / :1363)
// over device-resident polynomials.  A Go error is a C++ exception (hering::Error, carrying the library's status code and
// message); nothing here computes: every method is one call of the C ABI.  Objects are cheap shared references to library
// handles (a copy is another reference, as a Go pointer would be); the handle is released with the last reference.
//
// tests/cpp/parity.cpp is written against this header and reads like the reference's own ring_test.go / rlwe_test.go cases.
#ifndef HERING_HPP
#define HERING_HPP

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <functional>
#include <complex>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "hering.h"
#include "hering_ringswitch.h"
#include "hering_ringpack.h"
#include "hering_rgsw.h"
#include "hering_blindrot.h"
#include "hering_bridge.h"
#include "hering_bfv.h"
#include "hering_ckks_encoder.h"
#include "hering_bgv_encoder.h"
#include "hering_sampler.h"
#include "hering_encryptor.h"
#include "hering_keygen.h"
#include "hering_rgsw_encryptor.h"
#include "hering_multiparty.h"
#include "hering_lintrans.h"
#include "hering_polyeval.h"
#include "hering_ckks_evaluator.h"

namespace hering {

struct Error : std::runtime_error {
    int code;
    explicit Error(int rc) : std::runtime_error(std::string("hering: ") + he_last_error()), code(rc) {}
};
inline void check(int rc) {
    if (rc != HE_OK) throw Error(rc);
}

namespace detail {
struct Box {
    he_handle h = 0;
    int (*destroy)(he_handle) = nullptr;
    Box(he_handle h_, int (*d)(he_handle)) : h(h_), destroy(d) {}
    Box(const Box &) = delete;
    Box &operator=(const Box &) = delete;
    ~Box() {
        if (h && destroy) destroy(h);
    }
};
using Ref = std::shared_ptr<Box>;
inline Ref own(he_handle h, int (*d)(he_handle)) { return std::make_shared<Box>(h, d); }
}  // namespace detail

// One HIP device + stream.  There is no CPU fallback: without a device the constructor throws (HE_EDEVICE).
class Context {
    detail::Ref r_;

public:
    explicit Context(int device = 0) {
        he_handle h = 0;
        check(he_ctx_create(device, &h));
        r_ = detail::own(h, he_ctx_destroy);
    }
    he_handle h() const { return r_->h; }
    void Sync() const { check(he_ctx_sync(h())); }
    // the submission queue of the context (hering.h, he_ctx_set_coalescing): concurrent single-ciphertext calls of any operator --
    // one thread per ciphertext, the reference's b.RunParallel shape -- become batched launches over the callers' own polynomials
    void SetCoalescing(int maxBatch = 64, int windowMicros = 30) const { check(he_ctx_set_coalescing(h(), maxBatch, windowMicros)); }
    // deferred submission (hering.h, he_ctx_set_deferred): queued calls return once filed, the context's dispatcher thread launches
    // them; a failed launch is reported by the next Sync().  depth = 0: back to calls that return once launched
    void SetDeferred(int depth = 8) const { check(he_ctx_set_deferred(h(), depth)); }
    static int DeviceCount() {
        int n = 0;
        check(he_device_count(&n));
        return n;
    }
    static std::string Version() { return he_version(); }
    // CU count, LDS bytes per CU, clock kHz, HBM bytes
    std::array<uint64_t, 4> DeviceInfo() const {
        std::array<uint64_t, 4> v{};
        check(he_device_info(h(), v.data()));
        return v;
    }
    // HIP-event stopwatch on the context's stream
    void TimerStart() const { check(he_timer_start(h())); }
    float TimerStop() const {
        float ms = 0;
        check(he_timer_stop(h(), &ms));
        return ms;
    }
};

// A captured sequence of calls on a Context (he_graph_*): Capture(f) records what f enqueues; Launch replays it as one enqueue.
// f must have run once before (plans, scratch) and must not upload, download or Sync; the polynomials it touches must outlive the graph.
class Graph {
    detail::Ref r_;

public:
    template <class F>
    Graph(const Context &ctx, F &&f) {
        check(he_graph_begin(ctx.h()));
        he_handle g = 0;
        try {
            f();
        } catch (...) {
            if (he_graph_end(ctx.h(), &g) == HE_OK) he_graph_destroy(g);  // leave the context usable
            throw;
        }
        check(he_graph_end(ctx.h(), &g));
        r_ = detail::own(g, he_graph_destroy);
    }
    void Launch() const { check(he_graph_launch(r_->h)); }
    int Nodes() const {
        int n = 0;
        check(he_graph_nodes(r_->h, &n));
        return n;
    }
};

class Ring;

// A batch of ring.Poly in HBM: [batch][limbs][N] uint64 (ring/poly.go:13-16 with a leading batch axis).
class Poly {
    detail::Ref r_;
    int limbs_ = 0, batch_ = 0, n_ = 0;
    friend class Ring;
    Poly(he_handle h, int limbs, int batch, int n) : r_(detail::own(h, he_poly_free)), limbs_(limbs), batch_(batch), n_(n) {}

public:
    Poly() = default;
    he_handle h() const { return r_ ? r_->h : 0; }
    int Level() const { return limbs_ - 1; }
    int N() const { return n_; }
    int Batch() const { return batch_; }
    size_t Words() const { return (size_t)batch_ * limbs_ * n_; }
    // host image [batch][limbs][N]
    void Upload(const uint64_t *src, size_t words) { check(he_poly_upload(h(), src, words)); }
    void Upload(const std::vector<uint64_t> &src) { Upload(src.data(), src.size()); }
    void Download(uint64_t *dst, size_t words) const { check(he_poly_download(h(), dst, words)); }
    std::vector<uint64_t> Download() const {
        std::vector<uint64_t> v(Words());
        Download(v.data(), v.size());
        return v;
    }
    void CopyLvl(int level, const Poly &src) { check(he_poly_copy(h(), src.h(), level)); }  // ring.Poly.CopyLvl
    void Zero() { check(he_poly_zero(h())); }
    // one row of Coeffs [][]uint64: limb `limb` of batch entry b (N words)
    void UploadLimb(int b, int limb, const uint64_t *src) { check(he_poly_upload_limb(h(), b, limb, src)); }
    void DownloadLimb(int b, int limb, uint64_t *dst) const { check(he_poly_download_limb(h(), b, limb, dst)); }
    // limbs 0..level of entries [srcB0, srcB0 + nb) of src -> entries [dstB0, dstB0 + nb) of this batch
    void CopyBatch(int dstB0, const Poly &src, int srcB0, int nb, int level) { check(he_poly_copy_batch(h(), dstB0, src.h(), srcB0, nb, level)); }
    // what the library itself says about the handle (limbs, batch, N)
    std::array<int, 3> Shape() const {
        std::array<int, 3> v{};
        check(he_poly_shape(h(), &v[0], &v[1], &v[2]));
        return v;
    }
    // device storage for transports that move device memory themselves (drains the context's stream first)
    std::pair<void *, size_t> DeviceBuffer() const {
        void *p = nullptr;
        size_t n = 0;
        check(he_poly_device_buffer(h(), &p, &n));
        return {p, n};
    }
};

// the table ring.AutomorphismNTTIndex returns (ring/automorphism.go:12-34), on the device
class AutomorphismIndex {
    detail::Ref r_;
    int n_ = 0;
    friend class Ring;

public:
    AutomorphismIndex() = default;
    he_handle h() const { return r_ ? r_->h : 0; }
    std::vector<uint64_t> Download() const {
        std::vector<uint64_t> v((size_t)n_);
        check(he_automorphism_index_download(h(), v.data()));
        return v;
    }
};

enum class RingType { Standard = 0, ConjugateInvariant = 1 };  // ring/ring.go:24-27

// ring.Ring: the moduli chain with its NTT tables, at a level (AtLevel returns a shallow copy, ring/ring.go:186).
class Ring {
    detail::Ref r_;
    Context ctx_;
    std::vector<uint64_t> moduli_;
    int logN_ = 0, level_ = 0;
    RingType type_ = RingType::Standard;

public:
    // ring.NewRingFromType (ring/ring.go:267): throws HE_EPARAM for a modulus that is not an NTT-friendly prime, repeated moduli ...
    Ring(const Context &ctx, int logN, std::vector<uint64_t> moduli, RingType type = RingType::Standard)
        : ctx_(ctx), moduli_(std::move(moduli)), logN_(logN), level_((int)moduli_.size() - 1), type_(type) {
        he_handle h = 0;
        if (type == RingType::Standard) check(he_ring_create(ctx.h(), logN, moduli_.data(), (int)moduli_.size(), &h));  // ring.NewRing
        else check(he_ring_create_type(ctx.h(), logN, (int)type, moduli_.data(), (int)moduli_.size(), &h));
        r_ = detail::own(h, he_ring_destroy);
    }
    he_handle h() const { return r_->h; }
    const Context &Ctx() const { return ctx_; }
    int N() const { return 1 << logN_; }
    int LogN() const { return logN_; }
    int Level() const { return level_; }
    int MaxLevel() const { return (int)moduli_.size() - 1; }
    RingType Type() const { return type_; }
    const std::vector<uint64_t> &ModuliChain() const { return moduli_; }
    Ring AtLevel(int level) const {
        Ring c = *this;
        c.level_ = level;
        return c;
    }
    Poly NewPoly(int batch = 1) const {  // ring.Ring.NewPoly: zeroed, Level()+1 limbs
        he_handle h = 0;
        check(he_poly_alloc(this->h(), level_ + 1, batch, &h));
        return Poly(h, level_ + 1, batch, N());
    }
    Poly NewScratch(int batch = 1) const {  // not cleared: rlwe.BufferPool semantics (core/rlwe/pool.go)
        he_handle h = 0;
        check(he_poly_alloc_scratch(this->h(), level_ + 1, batch, &h));
        return Poly(h, level_ + 1, batch, N());
    }
    // SubRing constants (ring/subring.go:16-56): 0 Modulus, 1 MRedConstant, 2/3 BRedConstant, 4 NInv, 5 PrimitiveRoot
    uint64_t Constant(int limb, int which) const {
        uint64_t v = 0;
        check(he_ring_constant(h(), limb, which, &v));
        return v;
    }

    // ring/ntt.go:127-152
    void NTT(const Poly &p1, Poly &p2) const { check(he_ntt(h(), level_, p1.h(), p2.h())); }
    void NTTLazy(const Poly &p1, Poly &p2) const { check(he_ntt_lazy(h(), level_, p1.h(), p2.h())); }
    void INTT(const Poly &p1, Poly &p2) const { check(he_intt(h(), level_, p1.h(), p2.h())); }
    void INTTLazy(const Poly &p1, Poly &p2) const { check(he_intt_lazy(h(), level_, p1.h(), p2.h())); }

    // ring/operations.go
    void Add(const Poly &p1, const Poly &p2, Poly &p3) const { check(he_add(h(), level_, p1.h(), p2.h(), p3.h())); }
    void AddLazy(const Poly &p1, const Poly &p2, Poly &p3) const { bin(HE_ADD_LAZY, p1, p2, p3); }
    void Sub(const Poly &p1, const Poly &p2, Poly &p3) const { check(he_sub(h(), level_, p1.h(), p2.h(), p3.h())); }
    void SubLazy(const Poly &p1, const Poly &p2, Poly &p3) const { bin(HE_SUB_LAZY, p1, p2, p3); }
    void Neg(const Poly &p1, Poly &p2) const { check(he_neg(h(), level_, p1.h(), p2.h())); }
    void Reduce(const Poly &p1, Poly &p2) const { check(he_reduce(h(), level_, p1.h(), p2.h())); }
    void ReduceLazy(const Poly &p1, Poly &p2) const { un(HE_REDUCE_LAZY, p1, p2); }
    void MForm(const Poly &p1, Poly &p2) const { check(he_mform(h(), level_, p1.h(), p2.h())); }
    void MFormLazy(const Poly &p1, Poly &p2) const { un(HE_MFORM_LAZY, p1, p2); }
    void IMForm(const Poly &p1, Poly &p2) const { check(he_imform(h(), level_, p1.h(), p2.h())); }
    void MulCoeffsBarrett(const Poly &p1, const Poly &p2, Poly &p3) const { bin(HE_MUL_COEFFS_BARRETT, p1, p2, p3); }
    void MulCoeffsBarrettLazy(const Poly &p1, const Poly &p2, Poly &p3) const { bin(HE_MUL_COEFFS_BARRETT_LAZY, p1, p2, p3); }
    void MulCoeffsBarrettThenAdd(const Poly &p1, const Poly &p2, Poly &p3) const { bin(HE_MUL_COEFFS_BARRETT_THEN_ADD, p1, p2, p3); }
    void MulCoeffsBarrettThenAddLazy(const Poly &p1, const Poly &p2, Poly &p3) const { bin(HE_MUL_COEFFS_BARRETT_THEN_ADD_LAZY, p1, p2, p3); }
    void MulCoeffsMontgomery(const Poly &p1, const Poly &p2, Poly &p3) const { check(he_mul_coeffs_montgomery(h(), level_, p1.h(), p2.h(), p3.h())); }
    void MulCoeffsMontgomeryLazy(const Poly &p1, const Poly &p2, Poly &p3) const { check(he_mul_coeffs_montgomery_lazy(h(), level_, p1.h(), p2.h(), p3.h())); }
    void MulCoeffsMontgomeryLazyThenNeg(const Poly &p1, const Poly &p2, Poly &p3) const { bin(HE_MUL_COEFFS_MONTGOMERY_LAZY_THEN_NEG, p1, p2, p3); }
    void MulCoeffsMontgomeryThenAdd(const Poly &p1, const Poly &p2, Poly &p3) const { check(he_mul_coeffs_montgomery_then_add(h(), level_, p1.h(), p2.h(), p3.h())); }
    void MulCoeffsMontgomeryThenAddLazy(const Poly &p1, const Poly &p2, Poly &p3) const { bin(HE_MUL_COEFFS_MONTGOMERY_THEN_ADD_LAZY, p1, p2, p3); }
    void MulCoeffsMontgomeryLazyThenAddLazy(const Poly &p1, const Poly &p2, Poly &p3) const {
        check(he_mul_coeffs_montgomery_lazy_then_add_lazy(h(), level_, p1.h(), p2.h(), p3.h()));
    }
    void MulCoeffsMontgomeryThenSub(const Poly &p1, const Poly &p2, Poly &p3) const { bin(HE_MUL_COEFFS_MONTGOMERY_THEN_SUB, p1, p2, p3); }
    void MulCoeffsMontgomeryThenSubLazy(const Poly &p1, const Poly &p2, Poly &p3) const { bin(HE_MUL_COEFFS_MONTGOMERY_THEN_SUB_LAZY, p1, p2, p3); }
    void MulCoeffsMontgomeryLazyThenSubLazy(const Poly &p1, const Poly &p2, Poly &p3) const { bin(HE_MUL_COEFFS_MONTGOMERY_LAZY_THEN_SUB_LAZY, p1, p2, p3); }
    void AddScalar(const Poly &p1, uint64_t scalar, Poly &p2) const { sc(HE_ADD_SCALAR, p1, scalar, p2); }
    void SubScalar(const Poly &p1, uint64_t scalar, Poly &p2) const { sc(HE_SUB_SCALAR, p1, scalar, p2); }
    void MulScalar(const Poly &p1, uint64_t scalar, Poly &p2) const { sc(HE_MUL_SCALAR, p1, scalar, p2); }
    void MulScalarThenAdd(const Poly &p1, uint64_t scalar, Poly &p2) const { sc(HE_MUL_SCALAR_THEN_ADD, p1, scalar, p2); }
    void MulScalarThenSub(const Poly &p1, uint64_t scalar, Poly &p2) const { sc(HE_MUL_SCALAR_THEN_SUB, p1, scalar, p2); }
    void MulRNSScalarMontgomery(const Poly &p1, const std::vector<uint64_t> &scalar, Poly &p2) const {
        if ((int)scalar.size() <= level_) throw std::invalid_argument("MulRNSScalarMontgomery: one scalar per limb");
        check(he_mul_rns_scalar_montgomery(h(), level_, p1.h(), scalar.data(), p2.h()));
    }
    void Shift(const Poly &p1, int k, Poly &p2) const { check(he_shift(h(), level_, p1.h(), k, p2.h())); }
    void MultByMonomial(const Poly &p1, int k, Poly &p2) const { check(he_mult_by_monomial(h(), level_, p1.h(), k, p2.h())); }

    // ring/scaling.go
    void DivRoundByLastModulusNTT(const Poly &p0, Poly &p1) const { check(he_div_round_by_last_modulus_ntt(h(), level_, p0.h(), p1.h())); }
    void DivRoundByLastModulus(const Poly &p0, Poly &p1) const { check(he_div_round_by_last_modulus(h(), level_, p0.h(), p1.h())); }
    void DivFloorByLastModulusNTT(const Poly &p0, Poly &p1) const { check(he_div_floor_by_last_modulus_ntt(h(), level_, p0.h(), p1.h())); }
    void DivFloorByLastModulus(const Poly &p0, Poly &p1) const { check(he_div_floor_by_last_modulus(h(), level_, p0.h(), p1.h())); }
    void DivRoundByLastModulusManyNTT(int nbRescales, const Poly &p0, Poly &p1) const {
        check(he_div_round_by_last_modulus_many_ntt(h(), level_, nbRescales, p0.h(), p1.h()));
    }
    void DivRoundByLastModulusMany(int nbRescales, const Poly &p0, Poly &p1) const {
        check(he_div_round_by_last_modulus_many(h(), level_, nbRescales, p0.h(), p1.h()));
    }
    void DivFloorByLastModulusManyNTT(int nbRescales, const Poly &p0, Poly &p1) const {
        check(he_div_floor_by_last_modulus_many_ntt(h(), level_, nbRescales, p0.h(), p1.h()));
    }
    void DivFloorByLastModulusMany(int nbRescales, const Poly &p0, Poly &p1) const {
        check(he_div_floor_by_last_modulus_many(h(), level_, nbRescales, p0.h(), p1.h()));
    }

    // ring/automorphism.go: AutomorphismNTT (:36, not in place), Automorphism (:113, coefficient domain); galEl acts mod NthRoot.
    // Aliasing follows hering.h (Conventions): a pattern the C ABI rejects throws here before anything is launched.
    void AutomorphismNTT(const Poly &pIn, uint64_t galEl, Poly &pOut) const {
        he_handle ix = 0;
        check(he_automorphism_index_create(h(), galEl, &ix));
        detail::Ref keep = detail::own(ix, he_automorphism_index_destroy);
        check(he_automorphism_ntt_with_index(h(), level_, pIn.h(), ix, pOut.h()));
    }
    void Automorphism(const Poly &pIn, uint64_t galEl, Poly &pOut) const { check(he_automorphism(h(), level_, pIn.h(), galEl, pOut.h())); }
    // ring/conjugate_invariant.go:7,28 (hering_bridge.h): the maps between a standard polynomial of degree 2n and the compressed
    // conjugate-invariant one of degree n, on limbs 0..level of this ring.  The fold is the one of the index table of the Galois
    // element NthRoot - 1 (j -> 2n - 1 - j), the only one the reference passes; this ring supplies its moduli.
    void UnfoldConjugateInvariantToStandard(const Poly &polyConjugateInvariant, Poly &polyStandard) const {
        check(he_unfold_conjugate_invariant_to_standard(level_, polyConjugateInvariant.h(), polyStandard.h()));
    }
    void FoldStandardToConjugateInvariant(const Poly &polyStandard, Poly &polyConjugateInvariant) const {
        check(he_fold_standard_to_conjugate_invariant(h(), level_, polyStandard.h(), polyConjugateInvariant.h()));
    }
    AutomorphismIndex AutomorphismNTTIndex(uint64_t galEl) const {  // :12
        he_handle ix = 0;
        check(he_automorphism_index_create(h(), galEl, &ix));
        AutomorphismIndex a;
        a.r_ = detail::own(ix, he_automorphism_index_destroy);
        a.n_ = N();
        return a;
    }
    void AutomorphismNTTWithIndex(const Poly &pIn, const AutomorphismIndex &index, Poly &pOut) const {  // :50
        check(he_automorphism_ntt_with_index(h(), level_, pIn.h(), index.h(), pOut.h()));
    }
    void AutomorphismNTTWithIndexThenAddLazy(const Poly &pIn, const AutomorphismIndex &index, Poly &pOut) const {  // :82
        check(he_automorphism_ntt_with_index_then_add_lazy(h(), level_, pIn.h(), index.h(), pOut.h()));
    }
    // {Add,Sub,Mul}ScalarBigint, MulScalarBigintThenAdd (operations.go:158,193,231,240): little-endian 64-bit words of |scalar|
    void AddScalarBigint(const Poly &p1, const std::vector<uint64_t> &words, Poly &p2) const {
        check(he_add_scalar_bigint(h(), level_, p1.h(), words.data(), (int)words.size(), p2.h()));
    }
    void SubScalarBigint(const Poly &p1, const std::vector<uint64_t> &words, Poly &p2) const {
        check(he_sub_scalar_bigint(h(), level_, p1.h(), words.data(), (int)words.size(), p2.h()));
    }
    void MulScalarBigint(const Poly &p1, const std::vector<uint64_t> &words, Poly &p2) const {
        check(he_mul_scalar_bigint(h(), level_, p1.h(), words.data(), (int)words.size(), p2.h()));
    }
    void MulScalarBigintThenAdd(const Poly &p1, const std::vector<uint64_t> &words, Poly &p2) const {
        check(he_mul_scalar_bigint_then_add(h(), level_, p1.h(), words.data(), (int)words.size(), p2.h()));
    }
    // {Add,Sub,Mul}DoubleRNSScalar, MulDoubleRNSScalarThenAdd (operations.go:166,176,249,260): scalar0 on coefficients [0, N/2), scalar1 on [N/2, N)
    void AddDoubleRNSScalar(const Poly &p1, const std::vector<uint64_t> &s0, const std::vector<uint64_t> &s1, Poly &p2) const { drs(0, p1, s0, s1, p2); }
    void SubDoubleRNSScalar(const Poly &p1, const std::vector<uint64_t> &s0, const std::vector<uint64_t> &s1, Poly &p2) const { drs(1, p1, s0, s1, p2); }
    void MulDoubleRNSScalar(const Poly &p1, const std::vector<uint64_t> &s0, const std::vector<uint64_t> &s1, Poly &p2) const { drs(2, p1, s0, s1, p2); }
    void MulDoubleRNSScalarThenAdd(const Poly &p1, const std::vector<uint64_t> &s0, const std::vector<uint64_t> &s1, Poly &p2) const { drs(3, p1, s0, s1, p2); }
    // MulByVectorMontgomery / ...ThenAddLazy (operations.go:363,370): every limb times limb 0 of the batch-1 polynomial `vector`
    void MulByVectorMontgomery(const Poly &p1, const Poly &vector, Poly &p2) const { check(he_mul_by_vector_montgomery(h(), level_, p1.h(), vector.h(), 0, p2.h())); }
    void MulByVectorMontgomeryThenAddLazy(const Poly &p1, const Poly &vector, Poly &p2) const {
        check(he_mul_by_vector_montgomery(h(), level_, p1.h(), vector.h(), 1, p2.h()));
    }
    // SubRing.RootsForward / RootsBackward (ring/subring.go:44-47)
    std::vector<uint64_t> RootsForward(int limb) const { return roots(limb, 0); }
    std::vector<uint64_t> RootsBackward(int limb) const { return roots(limb, 1); }
    // ring.NumberTheoreticTransformer on host slices (ring/ntt.go:17-22): the plug point of ring.NewRingWithCustomNTT
    void Forward(int limb, const uint64_t *p1, uint64_t *p2) const { check(he_subring_ntt_host(h(), limb, 0, 0, p1, p2)); }
    void ForwardLazy(int limb, const uint64_t *p1, uint64_t *p2) const { check(he_subring_ntt_host(h(), limb, 0, 1, p1, p2)); }
    void Backward(int limb, const uint64_t *p1, uint64_t *p2) const { check(he_subring_ntt_host(h(), limb, 1, 0, p1, p2)); }
    void BackwardLazy(int limb, const uint64_t *p1, uint64_t *p2) const { check(he_subring_ntt_host(h(), limb, 1, 1, p1, p2)); }

    // the selector forms (enum he_binop / he_unop / he_scalarop of hering.h), for table-driven callers
    void BinOp(int op, const Poly &p1, const Poly &p2, Poly &p3) const { bin(op, p1, p2, p3); }
    void UnOp(int op, const Poly &p1, Poly &p2) const { un(op, p1, p2); }
    void ScalarOp(int op, const Poly &p1, uint64_t scalar, Poly &p2) const { sc(op, p1, scalar, p2); }

private:
    void drs(int op, const Poly &p1, const std::vector<uint64_t> &s0, const std::vector<uint64_t> &s1, Poly &p2) const {
        if ((int)s0.size() <= level_ || (int)s1.size() <= level_) throw std::invalid_argument("DoubleRNSScalar: one scalar pair per limb");
        check(he_double_rns_scalarop(h(), level_, op, p1.h(), s0.data(), s1.data(), p2.h()));
    }
    std::vector<uint64_t> roots(int limb, int dir) const {
        std::vector<uint64_t> v((size_t)N());
        check(he_ring_roots(h(), limb, dir, v.data()));
        return v;
    }
    void bin(int op, const Poly &p1, const Poly &p2, Poly &p3) const { check(he_binop(h(), level_, op, p1.h(), p2.h(), p3.h())); }
    void un(int op, const Poly &p1, Poly &p2) const { check(he_unop(h(), level_, op, p1.h(), p2.h())); }
    void sc(int op, const Poly &p1, uint64_t s, Poly &p2) const { check(he_scalarop(h(), level_, op, p1.h(), s, p2.h())); }
};

// ring.BasisExtender (ring/basis_extension.go:14)
class BasisExtender {
    detail::Ref r_;

public:
    BasisExtender(const Ring &ringQ, const Ring &ringP) {
        he_handle h = 0;
        check(he_basis_extender_create(ringQ.h(), ringP.h(), &h));
        r_ = detail::own(h, he_basis_extender_destroy);
    }
    he_handle h() const { return r_->h; }
    void ModUpQtoP(int levelQ, int levelP, const Poly &polQ, Poly &polP) const { check(he_modup_q_to_p(h(), levelQ, levelP, polQ.h(), polP.h())); }
    void ModUpPtoQ(int levelP, int levelQ, const Poly &polP, Poly &polQ) const { check(he_modup_p_to_q(h(), levelP, levelQ, polP.h(), polQ.h())); }
    void ModDownQPtoQ(int levelQ, int levelP, const Poly &p1Q, const Poly &p1P, Poly &p2Q) const {
        check(he_moddown_qp_to_q(h(), levelQ, levelP, p1Q.h(), p1P.h(), p2Q.h()));
    }
    void ModDownQPtoQNTT(int levelQ, int levelP, const Poly &p1Q, const Poly &p1P, Poly &p2Q) const {
        check(he_moddown_qp_to_q_ntt(h(), levelQ, levelP, p1Q.h(), p1P.h(), p2Q.h()));
    }
    void ModDownQPtoP(int levelQ, int levelP, const Poly &p1Q, const Poly &p1P, Poly &p2P) const {
        check(he_moddown_qp_to_p(h(), levelQ, levelP, p1Q.h(), p1P.h(), p2P.h()));
    }
};

// rlwe.Ciphertext: Value []ring.Poly (core/rlwe/ciphertext.go:13, element.go:27)
struct Ciphertext {
    std::vector<Poly> Value;
    int Degree() const { return (int)Value.size() - 1; }
    int Level() const { return Value.empty() ? -1 : Value[0].Level(); }
};
// ringqp.Poly{Q, P} (ring/ringqp/poly.go:17); a lazy key-switch result is two of them
struct PolyQP {
    Poly Q, P;
};

class Evaluator;

// rlwe.GadgetCiphertext in HBM (core/rlwe/gadgetciphertext.go:19-42): the payload of a RelinearizationKey / GaloisKey
class EvaluationKey {
    detail::Ref r_;
    int nQk_ = 0, nPk_ = 0;
    friend class Evaluator;

public:
    EvaluationKey() = default;
    he_handle h() const { return r_ ? r_->h : 0; }
    int LevelQ() const { return nQk_ - 1; }
    int LevelP() const { return nPk_ - 1; }
    // the key words back on the host: [beta][2][nQk + nPk][N]
    void Download(uint64_t *dst, size_t words) const { check(he_evk_download(h(), dst, words)); }
    // device storage for an external (GPU-to-GPU) fill; Commit() after the write has completed
    std::pair<void *, size_t> DeviceBuffer() const {
        void *p = nullptr;
        size_t n = 0;
        check(he_evk_device_buffer(h(), &p, &n));
        return {p, n};
    }
    void Commit() const { check(he_evk_commit(h())); }
};

// BuffDecompQP of Evaluator.DecomposeNTT: an opaque device buffer (beta digits of (Q limbs, P limbs) per batch entry)
class Decomposition {
    detail::Ref r_;
    friend class Evaluator;

public:
    Decomposition() = default;
    he_handle h() const { return r_ ? r_->h : 0; }
};

// rlwe.Evaluator's key-switch path + the two scheme call sites on top of it
class Evaluator {
    detail::Ref r_;
    Ring ringQ_, ringP_;

public:
    Evaluator(const Ring &ringQ, const Ring &ringP) : ringQ_(ringQ), ringP_(ringP) {
        he_handle h = 0;
        check(he_evaluator_create(ringQ.h(), ringP.h(), &h));
        r_ = detail::own(h, he_evaluator_destroy);
    }
    he_handle h() const { return r_->h; }
    const Ring &RingQ() const { return ringQ_; }
    const Ring &RingP() const { return ringP_; }

    // q: [beta][2][nQk][N], p: [beta][2][nPk][N], NTT + Montgomery form (what GenRelinearizationKeyNew / GenGaloisKeyNew produce)
    EvaluationKey NewEvaluationKey(int beta, int nQk, int nPk, const std::vector<uint64_t> &q, const std::vector<uint64_t> &p) const {
        const size_t n = (size_t)ringQ_.N();
        if (q.size() != (size_t)beta * 2 * nQk * n || p.size() != (size_t)beta * 2 * nPk * n)
            throw std::invalid_argument("NewEvaluationKey: host image size");
        he_handle h = 0;
        check(he_evk_create(this->h(), beta, nQk, nPk, q.data(), p.data(), &h));
        EvaluationKey k;
        k.r_ = detail::own(h, he_evk_destroy);
        k.nQk_ = nQk;
        k.nPk_ = nPk;
        return k;
    }
    // BaseTwoDecomposition = pw2 != 0 (at most one special prime; nPk = 0 and p empty: a key without P part): nj[i] bit windows of Q-limb i
    EvaluationKey NewEvaluationKeyBase2(int pw2, const std::vector<int> &nj, int nQk, int nPk, const std::vector<uint64_t> &q,
                                        const std::vector<uint64_t> &p) const {
        he_handle h = 0;
        check(he_evk_create_base2(this->h(), pw2, nj.data(), (int)nj.size(), nQk, nPk, q.data(), nPk > 0 ? p.data() : nullptr, &h));
        EvaluationKey k;
        k.r_ = detail::own(h, he_evk_destroy);
        k.nQk_ = nQk;
        k.nPk_ = nPk;
        return k;
    }
    // a zeroed key of that shape, to be generated on the device (rlwe::KeyGenerator) or filled through DeviceBuffer / Commit;
    // pw2 != 0: nj[i] bit windows of Q-limb i and beta = their sum
    EvaluationKey NewEvaluationKeyZero(int beta, int nQk, int nPk, int pw2 = 0, const std::vector<int> &nj = {}) const {
        he_handle h = 0;
        if (pw2) check(he_evk_create_base2(this->h(), pw2, nj.data(), (int)nj.size(), nQk, nPk, nullptr, nullptr, &h));
        else check(he_evk_create(this->h(), beta, nQk, nPk, nullptr, nullptr, &h));
        EvaluationKey k;
        k.r_ = detail::own(h, he_evk_destroy);
        k.nQk_ = nQk;
        k.nPk_ = nPk;
        return k;
    }
    Decomposition NewDecomposition(int batch = 1) const {
        he_handle h = 0;
        check(he_decomp_create(this->h(), batch, &h));
        Decomposition d;
        d.r_ = detail::own(h, he_decomp_destroy);
        return d;
    }

    // ---- rlwe.EvaluatorProvider (core/rlwe/rlwe.go:10-18) ----
    void DecomposeNTT(int levelQ, int levelP, int nbPi, const Poly &c2, bool c2IsNTT, Decomposition &decompQP) const {
        check(he_decompose_ntt(h(), levelQ, levelP, nbPi, c2.h(), c2IsNTT ? 1 : 0, decompQP.h()));
    }
    void GadgetProductLazy(int levelQ, const Poly &cx, const EvaluationKey &gadgetCt, std::array<PolyQP, 2> &ct) const {
        check(he_gadget_product_lazy(h(), levelQ, cx.h(), gadgetCt.h(), ct[0].Q.h(), ct[0].P.h(), ct[1].Q.h(), ct[1].P.h()));
    }
    void GadgetProductHoistedLazy(int levelQ, const Decomposition &decompQP, const EvaluationKey &gadgetCt, std::array<PolyQP, 2> &ct) const {
        check(he_gadget_product_hoisted_lazy(h(), levelQ, decompQP.h(), gadgetCt.h(), ct[0].Q.h(), ct[0].P.h(), ct[1].Q.h(), ct[1].P.h()));
    }
    void AutomorphismHoistedLazy(int levelQ, const Ciphertext &ctIn, const Decomposition &c1DecompQP, uint64_t galEl, const EvaluationKey &gk,
                                 std::array<PolyQP, 2> &ctQP) const {
        check(he_automorphism_hoisted_lazy(h(), levelQ, ctIn.Value.at(0).h(), c1DecompQP.h(), galEl, gk.h(), ctQP[0].Q.h(), ctQP[0].P.h(),
                                           ctQP[1].Q.h(), ctQP[1].P.h()));
    }
    void ModDownQPtoQNTT(int levelQ, int levelP, const Poly &p1Q, const Poly &p1P, Poly &p2Q) const {
        check(he_eval_moddown_qp_to_q_ntt(h(), levelQ, levelP, p1Q.h(), p1P.h(), p2Q.h()));
    }
    // (CheckAndGetGaloisKey / AutomorphismIndex are key-set and table look-ups of the Go side: go/hering/evaluator.go)

    // Decomposer.DecomposeAndSplit (ring/basis_extension.go:381): coefficient-domain p0Q -> digit `digit` extended to (p1Q, p1P)
    void DecomposeAndSplit(int levelQ, int levelP, int nbPi, int digit, const Poly &p0Q, Poly &p1Q, Poly &p1P) const {
        check(he_decompose_and_split(h(), levelQ, levelP, nbPi, digit, p0Q.h(), p1Q.h(), p1P.h()));
    }
    // the inner product over the digits [digitBegin, digitEnd) only (a key switch split over GPUs by digit)
    void GadgetProductHoistedLazyDigits(int levelQ, const Decomposition &decompQP, const EvaluationKey &gadgetCt, int digitBegin, int digitEnd,
                                        std::array<PolyQP, 2> &ct) const {
        check(he_gadget_product_hoisted_lazy_digits(h(), levelQ, decompQP.h(), gadgetCt.h(), digitBegin, digitEnd, ct[0].Q.h(), ct[0].P.h(),
                                                    ct[1].Q.h(), ct[1].P.h()));
    }
    // one limb of the hoisting buffer back on the host (tests)
    void DecompositionLimb(const Decomposition &d, int b, int digit, bool isP, int limb, uint64_t *dst) const {
        check(he_decomp_download_limb(d.h(), b, digit, isP ? 1 : 0, limb, dst));
    }
    // pieces of bootstrapping.Evaluator.ModUp (circuits/ckks/bootstrapping/evaluator.go:654-755)
    void CenteredLift(int strict, const Poly &src, int firstQ, int levelQ, Poly &dstQ, int levelP, Poly &dstP) const {
        check(he_centered_lift(h(), strict, src.h(), firstQ, levelQ, dstQ.h(), levelP, dstP.h()));
    }
    void DecompositionFill(Decomposition &d, int levelQ, int levelP, const Poly &srcQ, const Poly &srcP) const {
        check(he_decomp_fill(d.h(), levelQ, levelP, srcQ.h(), srcP.h()));
    }
    // inner accumulation of lintrans.Evaluator.MultiplyByDiagMatrix[BSGS] (lintrans_evaluator.go:216-241, :346-394): term i =
    // (plaintext diagonal, ciphertext, optional automorphism index); out_k = Reduce([out_k +] sum_i pt_i * phi_i(ct_i[k])) on Q and P
    struct DiagTerm {
        PolyQP pt, c0, c1;             // c0.P / c1.P empty: the term has no P part
        const AutomorphismIndex *index;  // nullptr: no automorphism
    };
    void LinTransMulSum(int levelQ, int levelP, const std::vector<DiagTerm> &terms, bool accumulate, std::array<PolyQP, 2> &out) const {
        const int n = (int)terms.size();
        std::vector<he_handle> ptQ(n), ptP(n), c0Q(n), c0P(n), c1Q(n), c1P(n), ix(n);
        bool any_index = false;
        for (int i = 0; i < n; i++) {
            ptQ[i] = terms[i].pt.Q.h(); ptP[i] = terms[i].pt.P.h();
            c0Q[i] = terms[i].c0.Q.h(); c0P[i] = terms[i].c0.P.h();
            c1Q[i] = terms[i].c1.Q.h(); c1P[i] = terms[i].c1.P.h();
            ix[i] = terms[i].index ? terms[i].index->h() : 0;
            any_index = any_index || ix[i] != 0;
        }
        check(he_lintrans_mul_sum(h(), levelQ, levelP, n, ptQ.data(), ptP.data(), c0Q.data(), c0P.data(), c1Q.data(), c1P.data(),
                                  any_index ? ix.data() : nullptr, accumulate ? 1 : 0, out[0].Q.h(), out[0].P.h(), out[1].Q.h(), out[1].P.h()));
    }

    // the giant step of lintrans.Evaluator.MultiplyByDiagMatrixBSGS (lintrans_evaluator.go:397-441) as one call: GadgetProductLazy(cx)
    // -> cQP; cQP[0] += add; out[k] (+)= AutomorphismNTTWithIndex[ThenAddLazy](cQP[k]) -- the key inner products store through
    // the automorphism themselves (he_lintrans_giant_step)
    void LinTransGiantStep(int levelQ, const Poly &cx, const EvaluationKey &galoisKey, uint64_t galEl, const PolyQP &add, bool accumulate,
                           std::array<PolyQP, 2> &out) const {
        check(he_lintrans_giant_step(h(), levelQ, cx.h(), galoisKey.h(), galEl, add.Q.h(), add.P.h(), out[0].Q.h(), out[0].P.h(), out[1].Q.h(),
                                     out[1].P.h(), accumulate ? 1 : 0));
    }

    // ---- rlwe.Evaluator ----
    void ModDown(int levelQ, int levelP, const std::array<PolyQP, 2> &ctQP, Ciphertext &ct) const {
        check(he_moddown(h(), levelQ, levelP, ctQP[0].Q.h(), ctQP[0].P.h(), ctQP[1].Q.h(), ctQP[1].P.h(), ct.Value.at(0).h(), ct.Value.at(1).h()));
    }
    void GadgetProduct(int levelQ, const Poly &cx, const EvaluationKey &gadgetCt, Ciphertext &ct) const {
        check(he_gadget_product(h(), levelQ, cx.h(), gadgetCt.h(), ct.Value.at(0).h(), ct.Value.at(1).h()));
    }
    void GadgetProductHoisted(int levelQ, const Decomposition &decompQP, const EvaluationKey &gadgetCt, Ciphertext &ct) const {
        check(he_gadget_product_hoisted(h(), levelQ, decompQP.h(), gadgetCt.h(), ct.Value.at(0).h(), ct.Value.at(1).h()));
    }
    void Relinearize(const Ciphertext &ctIn, const EvaluationKey &rlk, Ciphertext &opOut) const {  // evaluator_evaluationkey.go:117
        if (ctIn.Degree() != 2) throw std::invalid_argument("cannot relinearize: ctIn.Degree() should be 2 but is " + std::to_string(ctIn.Degree()));
        check(he_relinearize(h(), ctIn.Level(), ctIn.Value[0].h(), ctIn.Value[1].h(), ctIn.Value[2].h(), rlk.h(), opOut.Value.at(0).h(),
                             opOut.Value.at(1).h()));
    }
    // evaluator_evaluationkey.go:36-106: ctIn and opOut of the evaluator's degree, or one of them of a smaller degree (NTT domain)
    void ApplyEvaluationKey(const Ciphertext &ctIn, const EvaluationKey &evk, Ciphertext &opOut) const {
        if (ctIn.Degree() != 1 || opOut.Degree() != 1)
            throw std::invalid_argument("cannot ApplyEvaluationKey: input and output Ciphertext must be of degree 1");
        const int level = ctIn.Level() < opOut.Level() ? ctIn.Level() : opOut.Level();
        check(he_apply_evaluation_key(h(), level, ctIn.Value[0].h(), ctIn.Value[1].h(), evk.h(), opOut.Value[0].h(), opOut.Value[1].h()));
    }
    void Automorphism(const Ciphertext &ctIn, uint64_t galEl, const EvaluationKey &gk, Ciphertext &opOut) const {  // evaluator_automorphism.go:13
        check(he_automorphism_ct(h(), ctIn.Level(), ctIn.Value.at(0).h(), ctIn.Value.at(1).h(), galEl, gk.h(), opOut.Value.at(0).h(),
                                 opOut.Value.at(1).h()));
    }
    void AutomorphismHoisted(int level, const Ciphertext &ctIn, const Decomposition &c1DecompQP, uint64_t galEl, const EvaluationKey &gk,
                             Ciphertext &opOut) const {  // :60
        check(he_automorphism_hoisted(h(), level, ctIn.Value.at(0).h(), c1DecompQP.h(), galEl, gk.h(), opOut.Value.at(0).h(), opOut.Value.at(1).h()));
    }

    // ---- schemes: degree 1 x degree 1.  relin = false: the degree-2 result (opOut needs three components) ----
    void MulRelinCKKS(const Ciphertext &op0, const Ciphertext &op1, const EvaluationKey *rlk, Ciphertext &opOut) const {
        mul(false, 0, op0, op1, rlk, opOut);
    }
    void MulRelinBGV(uint64_t t, const Ciphertext &op0, const Ciphertext &op1, const EvaluationKey *rlk, Ciphertext &opOut) const {
        mul(true, t, op0, op1, rlk, opOut);
    }
    // Evaluator.Rescale: DivRoundByLastModulusManyNTT per component (schemes/ckks/evaluator.go:477, schemes/bgv/evaluator.go:1363)
    void Rescale(int nbRescales, const Ciphertext &op0, Ciphertext &opOut) const {
        std::vector<he_handle> in, out;
        for (size_t i = 0; i < op0.Value.size(); i++) { in.push_back(op0.Value[i].h()); out.push_back(opOut.Value.at(i).h()); }
        check(he_rescale_polys(ringQ_.h(), op0.Level(), nbRescales, (int)in.size(), in.data(), out.data()));  // the loop as one call
    }
    // the reference's parallel mode (many goroutines, one ciphertext per call) gathered into batched launches: hering.h
    // (the queue belongs to the evaluator's context and serves every operator of that context: Context::SetCoalescing is the same switch)
    void SetCoalescing(int maxBatch = 64, int windowMicros = 30) const { check(he_evaluator_set_coalescing(h(), maxBatch, windowMicros)); }

private:
    void mul(bool bgv, uint64_t t, const Ciphertext &op0, const Ciphertext &op1, const EvaluationKey *rlk, Ciphertext &opOut) const {
        if (op0.Degree() != 1 || op1.Degree() != 1) throw std::invalid_argument("MulRelin: operands of degree 1");
        const he_handle k = rlk ? rlk->h() : 0, o2 = rlk ? 0 : opOut.Value.at(2).h();
        const int level = op0.Level() < op1.Level() ? op0.Level() : op1.Level();
        if (bgv)
            check(he_bgv_mul_relin(h(), level, t, op0.Value[0].h(), op0.Value[1].h(), op1.Value[0].h(), op1.Value[1].h(), k, opOut.Value.at(0).h(),
                                   opOut.Value.at(1).h(), o2));
        else
            check(he_ckks_mul_relin(h(), level, op0.Value[0].h(), op0.Value[1].h(), op1.Value[0].h(), op1.Value[1].h(), k, opOut.Value.at(0).h(),
                                    opOut.Value.at(1).h(), o2));
    }
};

// ring.MapSmallDimensionToLargerDimensionNTT (ring/operations.go:380)
inline void MapSmallDimensionToLargerDimensionNTT(const Poly &polSmall, Poly &polLarge) {
    check(he_map_small_to_large_ntt(polSmall.h(), polLarge.h(), polSmall.Level() < polLarge.Level() ? polSmall.Level() : polLarge.Level()));
}
// rlwe.SwitchCiphertextRingDegreeNTT (core/rlwe/element.go:250): ringQLargeDim is required for large -> small (nullptr otherwise)
inline void SwitchCiphertextRingDegreeNTT(const Ciphertext &ctIn, const Ring *ringQLargeDim, Ciphertext &opOut) {
    for (size_t i = 0; i < opOut.Value.size(); i++) {
        const Poly &a = ctIn.Value.at(i), &b = opOut.Value[i];
        check(he_switch_ring_degree_ntt(ringQLargeDim ? ringQLargeDim->h() : 0, a.Level() < b.Level() ? a.Level() : b.Level(), a.h(), b.h()));
    }
}
// rlwe.SwitchCiphertextRingDegree (core/rlwe/element.go:293), coefficient domain
inline void SwitchCiphertextRingDegree(const Ciphertext &ctIn, Ciphertext &opOut) {
    for (size_t i = 0; i < opOut.Value.size(); i++) {
        const Poly &a = ctIn.Value.at(i), &b = opOut.Value[i];
        check(he_switch_ring_degree(a.Level() < b.Level() ? a.Level() : b.Level(), a.h(), b.h()));
    }
}

// ---- ring packing (core/rlwe/ring_packing.go; hering_ringpack.h), standard rings, NTT domain -----------------------------------
namespace detail {
inline std::vector<he_handle> handles(const std::vector<const Poly *> &v) {
    std::vector<he_handle> h(v.size());
    for (size_t i = 0; i < v.size(); i++) h[i] = v[i] ? v[i]->h() : 0;
    return h;
}
}  // namespace detail
// GenXPow2NTT(ring.AtLevel(level), logN, div)[i] (:772-810), read off the resident twiddle tables
inline void XPow2NTT(const Ring &ring, int level, int i, bool div, Poly &out) { check(he_ring_xpow2_ntt(ring.h(), level, i, div ? 1 : 0, out.h())); }
// the ring maps of Split (:205-225) / Merge (:410-417) on one polynomial; the odd operand may be nullptr
inline void SplitNTT(const Ring &ringLarge, int level, const Poly &in, Poly &outEven, Poly *outOdd) {
    check(he_ring_split_ntt(ringLarge.h(), level, in.h(), outEven.h(), outOdd ? outOdd->h() : 0));
}
inline void MergeNTT(const Ring &ringLarge, int level, const Poly &inEven, const Poly *inOdd, Poly &out) {
    check(he_ring_merge_ntt(ringLarge.h(), level, inEven.h(), inOdd ? inOdd->h() : 0, out.h()));
}
// Expand's inner step at n = 2^k (:528-559) over batched ciphertexts: out of 2 m entries, or m (and possibly in itself) when sumOnly
inline void ExpandStep(const Ring &ring, int level, int k, bool sumOnly, const Ciphertext &in, const Ciphertext &tmp, Ciphertext &out) {
    check(he_ringpack_expand_step(ring.h(), level, k, sumOnly ? 1 : 0, in.Value.at(0).h(), in.Value.at(1).h(), tmp.Value.at(0).h(),
                                  tmp.Value.at(1).h(), out.Value.at(0).h(), out.Value.at(1).h()));
}
// Pack's inner step (:697-765) before / after the automorphism of T, over pairs of single ciphertexts (nullptr: absent)
inline void PackPre(const Ring &ring, int level, int k, const std::vector<const Poly *> &a0, const std::vector<const Poly *> &a1,
                    const std::vector<const Poly *> &b0, const std::vector<const Poly *> &b1, Ciphertext &T) {
    const std::vector<he_handle> ha0 = detail::handles(a0), ha1 = detail::handles(a1), hb0 = detail::handles(b0), hb1 = detail::handles(b1);
    if (ha0.empty() || ha1.size() != ha0.size() || hb0.size() != ha0.size() || hb1.size() != ha0.size()) throw std::invalid_argument("PackPre: pair lists of different length");
    check(he_ringpack_pack_pre(ring.h(), level, k, (int)ha0.size(), ha0.data(), ha1.data(), hb0.data(), hb1.data(), T.Value.at(0).h(), T.Value.at(1).h()));
}
inline void PackPost(const Ring &ring, int level, const std::vector<const Poly *> &a0, const std::vector<const Poly *> &a1,
                     const std::vector<const Poly *> &b0, const std::vector<const Poly *> &b1, Ciphertext &T) {
    const std::vector<he_handle> ha0 = detail::handles(a0), ha1 = detail::handles(a1), hb0 = detail::handles(b0), hb1 = detail::handles(b1);
    if (ha0.empty() || ha1.size() != ha0.size() || hb0.size() != ha0.size() || hb1.size() != ha0.size()) throw std::invalid_argument("PackPost: pair lists of different length");
    check(he_ringpack_pack_post(ring.h(), level, (int)ha0.size(), ha0.data(), ha1.data(), hb0.data(), hb1.data(), T.Value.at(0).h(), T.Value.at(1).h()));
}
// rlwe.RingPackingEvaluator (:13): Split and Merge between the degree N of `evalN` and N/2; ringQNHalf allocates the halves
class RingPackingEvaluator {
    Evaluator evalN_;  // (a copy shares the device evaluator, as every mirror class shares its handle)
    Ring ringQNHalf_;
    EvaluationKey evkNToNHalf_, evkNHalfToN_;

public:
    RingPackingEvaluator(const Evaluator &evalN, const Ring &ringQNHalf, const EvaluationKey &evkNToNHalf, const EvaluationKey &evkNHalfToN)
        : evalN_(evalN), ringQNHalf_(ringQNHalf), evkNToNHalf_(evkNToNHalf), evkNHalfToN_(evkNHalfToN) {
        if (ringQNHalf.N() * 2 != evalN.RingQ().N()) throw std::invalid_argument("RingPackingEvaluator: ringQNHalf is not of degree N/2");
    }
    // :173-228; ctOddNHalf may be nullptr
    void Split(const Ciphertext &ctN, Ciphertext &ctEvenNHalf, Ciphertext *ctOddNHalf) const {
        check(he_ringpack_split(evalN_.h(), ctN.Level(), ctN.Value.at(0).h(), ctN.Value.at(1).h(), evkNToNHalf_.h(), ctEvenNHalf.Value.at(0).h(),
                                ctEvenNHalf.Value.at(1).h(), ctOddNHalf ? ctOddNHalf->Value.at(0).h() : 0, ctOddNHalf ? ctOddNHalf->Value.at(1).h() : 0));
    }
    std::pair<Ciphertext, Ciphertext> SplitNew(const Ciphertext &ctN) const {
        const Ring r = ringQNHalf_.AtLevel(ctN.Level());
        const int B = ctN.Value.at(0).Batch();
        Ciphertext even{{r.NewPoly(B), r.NewPoly(B)}}, odd{{r.NewPoly(B), r.NewPoly(B)}};
        Split(ctN, even, &odd);
        return {even, odd};
    }
    // :376-426; ctOddNHalf may be nullptr
    void Merge(const Ciphertext &ctEvenNHalf, const Ciphertext *ctOddNHalf, Ciphertext &ctN) const {
        check(he_ringpack_merge(evalN_.h(), ctN.Level(), ctEvenNHalf.Value.at(0).h(), ctEvenNHalf.Value.at(1).h(),
                                ctOddNHalf ? ctOddNHalf->Value.at(0).h() : 0, ctOddNHalf ? ctOddNHalf->Value.at(1).h() : 0, evkNHalfToN_.h(),
                                ctN.Value.at(0).h(), ctN.Value.at(1).h()));
    }
    Ciphertext MergeNew(const Ciphertext &ctEvenNHalf, const Ciphertext *ctOddNHalf) const {
        const Ring r = evalN_.RingQ().AtLevel(ctEvenNHalf.Level());
        const int B = ctEvenNHalf.Value.at(0).Batch();
        Ciphertext ctN{{r.NewPoly(B), r.NewPoly(B)}};
        Merge(ctEvenNHalf, ctOddNHalf, ctN);
        return ctN;
    }
};

// ---- the CKKS bridge (schemes/ckks/bridge.go; hering_bridge.h), NTT domain ---------------------------------------------------------
namespace ckks {
// ckks.DomainSwitcher (bridge.go:13): between standard ciphertexts of the evaluator's degree N and conjugate-invariant ones of
// degree N/2.  Either key may be absent (a default EvaluationKey).  hering::Ciphertext carries no scale: after ComplexToReal the
// caller doubles the scale it keeps for the ciphertext (bridge.go:93).
class DomainSwitcher {
    Evaluator eval_;  // (a copy shares the device evaluator)
    EvaluationKey stdToci_, ciToStd_;

public:
    DomainSwitcher(const Evaluator &eval, const EvaluationKey &comlexToRealEvk, const EvaluationKey &realToComplexEvk)
        : eval_(eval), stdToci_(comlexToRealEvk), ciToStd_(realToComplexEvk) {}
    void ComplexToReal(const Ciphertext &ctIn, Ciphertext &opOut) const {  // :57-95
        if (!stdToci_.h()) throw std::invalid_argument("cannot ComplexToReal: no realToComplexEvk provided to this DomainSwitcher");
        const int level = ctIn.Level() < opOut.Level() ? ctIn.Level() : opOut.Level();
        check(he_complex_to_real(eval_.h(), level, ctIn.Value.at(0).h(), ctIn.Value.at(1).h(), stdToci_.h(), opOut.Value.at(0).h(), opOut.Value.at(1).h()));
    }
    void RealToComplex(const Ciphertext &ctIn, Ciphertext &opOut) const {  // :104-144
        if (!ciToStd_.h()) throw std::invalid_argument("cannot RealToComplex: no realToComplexEvk provided to this DomainSwitcher");
        const int level = ctIn.Level() < opOut.Level() ? ctIn.Level() : opOut.Level();
        check(he_real_to_complex(eval_.h(), level, ctIn.Value.at(0).h(), ctIn.Value.at(1).h(), ciToStd_.h(), opOut.Value.at(0).h(), opOut.Value.at(1).h()));
    }
};

// ckks.Encoder, the double-precision path (schemes/ckks/encoder.go, prec <= 53; hering_ckks_encoder.h).  A plaintext is a Poly
// plus the fields of rlwe.MetaData the reference reads; vectors are std::vector<std::complex<double>> or std::vector<double>,
// [batch][n] flattened (batch = the polynomial's).
struct MetaData {
    double Scale = 1.0;
    int LogSlots = 0;  // LogDimensions.Cols
    bool IsBatched = true, IsNTT = true, IsMontgomery = false;
};
class Encoder {
    detail::Ref r_;
    int info_[4] = {0, 0, 0, 0};
    static const double *dp(const std::vector<std::complex<double>> &v) { return reinterpret_cast<const double *>(v.data()); }
    static double *dp(std::vector<std::complex<double>> &v) { return reinterpret_cast<double *>(v.data()); }

public:
    // NewEncoder (:78): ringP for EncodeQP only; roots: empty for the built-in table, or NthRoot + 1 values
    explicit Encoder(const Ring &ringQ, const Ring *ringP = nullptr, const std::vector<std::complex<double>> &roots = {}) {
        if (!roots.empty() && roots.size() != (size_t)(ringQ.Type() == RingType::Standard ? 2 : 4) * ringQ.N() + 1)
            throw std::invalid_argument("ckks::Encoder: the table of roots must hold NthRoot + 1 values");
        he_handle h = 0;
        check(he_ckks_encoder_create(ringQ.h(), ringP ? ringP->h() : 0, roots.empty() ? nullptr : dp(roots), &h));
        r_ = detail::own(h, he_ckks_encoder_destroy);
        check(he_ckks_encoder_info(h, info_));
    }
    he_handle h() const { return r_->h; }
    int LogMaxSlots() const { return info_[1]; }
    int FFTOneWorkgroupMaxLogN() const { return info_[2]; }
    int DecodeMaxLimbs() const { return info_[3]; }
    // GetRootsComplex128 (utils.go:53) on the host, and the table this encoder holds
    static std::vector<std::complex<double>> RootsHost(uint64_t nthRoot) {
        std::vector<std::complex<double>> out(nthRoot + 1);
        check(he_ckks_roots_host(nthRoot, dp(out)));
        return out;
    }
    std::vector<std::complex<double>> Roots() const {
        std::vector<std::complex<double>> out(((size_t)1 << info_[0]) + 1);
        check(he_ckks_encoder_roots(h(), dp(out)));
        return out;
    }
    // Encoder.FFT / IFFT (:765-820), in place, values.size() = batch << logN
    void FFT(std::vector<std::complex<double>> &values, int logN) const { check(he_ckks_fft(h(), logN, (int)(values.size() >> logN), dp(values))); }
    void IFFT(std::vector<std::complex<double>> &values, int logN) const { check(he_ckks_ifft(h(), logN, (int)(values.size() >> logN), dp(values))); }
    // Encoder.Encode (:156): values.size() / pt.Batch() values per entry
    void Encode(const std::vector<std::complex<double>> &values, const MetaData &m, Poly &pt) const {
        check(he_ckks_encode(h(), pt.Level(), m.LogSlots, m.Scale, m.IsBatched, m.IsNTT, m.IsMontgomery, dp(values), values.size() / pt.Batch(), 1,
                             pt.Batch(), pt.h()));
    }
    void Encode(const std::vector<double> &values, const MetaData &m, Poly &pt) const {
        check(he_ckks_encode(h(), pt.Level(), m.LogSlots, m.Scale, m.IsBatched, m.IsNTT, m.IsMontgomery, values.data(), values.size() / pt.Batch(), 0,
                             pt.Batch(), pt.h()));
    }
    // Encoder.Embed (:208) into a ring.Poly: the batched arm of Encode; into a ringqp.Poly (:321-328): EncodeQP
    void Embed(const std::vector<std::complex<double>> &values, MetaData m, Poly &polyOut) const {
        m.IsBatched = true;
        Encode(values, m, polyOut);
    }
    void EncodeQP(const std::vector<std::complex<double>> &values, const MetaData &m, Poly &polyQ, Poly &polyP) const {
        check(he_ckks_encode_qp(h(), polyQ.Level(), polyP.Level(), m.LogSlots, m.Scale, m.IsNTT, m.IsMontgomery, dp(values),
                                values.size() / polyQ.Batch(), 1, polyQ.Batch(), polyQ.h(), polyP.h()));
    }
    // Encoder.DecodePublic (:199): [batch][slots] complex values ([batch][N] when the plaintext is not batched)
    std::vector<std::complex<double>> DecodePublic(const Poly &pt, const MetaData &m, double logprec) const {
        std::vector<std::complex<double>> out((size_t)pt.Batch() * (m.IsBatched ? (size_t)1 << m.LogSlots : (size_t)pt.N()));
        check(he_ckks_decode(h(), pt.Level(), m.LogSlots, m.Scale, m.IsBatched, m.IsNTT, logprec, pt.h(), 1, dp(out)));
        return out;
    }
    std::vector<std::complex<double>> Decode(const Poly &pt, const MetaData &m) const { return DecodePublic(pt, m, 0.0); }
};
}  // namespace ckks

// ---- BFV (schemes/bgv/evaluator.go with ScaleInvariant = true; hering_bfv.h), NTT domain ----------------------------------------
namespace bgv {
// bgv.Evaluator restricted to the scale-invariant ct x ct multiplication: newEvaluatorPrecomp (:38-70) over the device evaluator of
// the parameters, Parameters.RingQMul() and the plaintext modulus; `rlk` as the reference's evaluation key set holds it (a default
// EvaluationKey: none).  hering::Ciphertext carries no scale: the caller records MulScaleInvariant(params, a, b, level) (:983).
class Evaluator {
    detail::Ref r_;
    hering::Evaluator eval_;  // (a copy shares the device evaluator)
    Ring ringQMul_;
    EvaluationKey rlk_;
    std::vector<int> levelQMul_;

    void tensor(const Ciphertext &op0, const Ciphertext &op1, bool relin, Ciphertext &opOut) const {
        if (op0.Degree() != 1 || op1.Degree() != 1)
            throw std::invalid_argument("cannot MulScaleInvariant: input elements total degree cannot be larger than 2");  // :831
        if (relin && !rlk_.h()) throw std::invalid_argument("cannot relinearize: no relinearization key");
        int level = op0.Level() < op1.Level() ? op0.Level() : op1.Level();
        if (opOut.Level() < level) level = opOut.Level();  // :810
        check(he_bfv_mul_relin(h(), level, op0.Value[0].h(), op0.Value[1].h(), op1.Value[0].h(), op1.Value[1].h(), relin ? rlk_.h() : 0,
                               opOut.Value.at(0).h(), opOut.Value.at(1).h(), relin ? 0 : opOut.Value.at(2).h()));
    }

public:
    Evaluator(const hering::Evaluator &eval, const Ring &ringQMul, uint64_t t, const EvaluationKey &rlk = EvaluationKey())
        : eval_(eval), ringQMul_(ringQMul), rlk_(rlk) {
        he_handle h = 0;
        check(he_bfv_evaluator_create(eval.h(), ringQMul.h(), t, &h));
        r_ = detail::own(h, he_bfv_evaluator_destroy);
        for (int level = 0; level <= eval.RingQ().MaxLevel(); level++) {
            int lm = 0;
            check(he_bfv_level_qmul(h, level, &lm));
            levelQMul_.push_back(lm);
        }
    }
    he_handle h() const { return r_->h; }
    const std::vector<int> &LevelQMul() const { return levelQMul_; }
    // MulScaleInvariant (:799): the degree-2 result, opOut of three components
    void MulScaleInvariant(const Ciphertext &op0, const Ciphertext &op1, Ciphertext &opOut) const { tensor(op0, op1, false, opOut); }
    // MulRelinScaleInvariant (:838)
    void MulRelinScaleInvariant(const Ciphertext &op0, const Ciphertext &op1, Ciphertext &opOut) const { tensor(op0, op1, true, opOut); }
    // quantize (:1050) as a piece: c2Q1 on Q, c2Q2 on QMul at levelQMul, NTT domain; the result replaces c2Q1 as in the reference
    void Quantize(int level, Poly &c2Q1, const Poly &c2Q2) const { check(he_bfv_quantize(h(), level, c2Q1.h(), c2Q2.h(), c2Q1.h())); }
};

// bgv.Encoder (schemes/bgv/encoder.go; hering_bgv_encoder.h).  A plaintext is a Poly plus the fields of rlwe.MetaData the reference
// reads; value vectors are std::vector<uint64_t> ([]uint64) or std::vector<int64_t> ([]int64), [batch][n] flattened (batch = the
// polynomial's); decoded vectors are [batch][MaxSlots].
struct MetaData {
    uint64_t Scale = 1;
    bool IsBatched = true, IsNTT = true, IsMontgomery = false;
};
class Encoder {
    detail::Ref r_;
    int info_[4] = {0, 0, 0, 0};
    static const uint64_t *up(const std::vector<uint64_t> &v) { return v.data(); }
    static const uint64_t *up(const std::vector<int64_t> &v) { return reinterpret_cast<const uint64_t *>(v.data()); }
    static uint64_t *up(std::vector<uint64_t> &v) { return v.data(); }
    static uint64_t *up(std::vector<int64_t> &v) { return reinterpret_cast<uint64_t *>(v.data()); }
    template <class V> static constexpr int is_signed() { return std::is_same<typename V::value_type, int64_t>::value ? 1 : 0; }

public:
    // NewEncoder (:49): ringT = Parameters.RingT(); ringP for EncodeQP and RingT2Q into ringP only
    Encoder(const Ring &ringQ, const Ring &ringT, const Ring *ringP = nullptr) {
        he_handle h = 0;
        check(he_bgv_encoder_create(ringQ.h(), ringP ? ringP->h() : 0, ringT.h(), &h));
        r_ = detail::own(h, he_bgv_encoder_destroy);
        check(he_bgv_encoder_info(h, info_));
    }
    he_handle h() const { return r_->h; }
    int LogMaxSlots() const { return info_[0]; }
    int MaxSlots() const { return 1 << info_[0]; }
    int LogGap() const { return info_[1]; }
    int RingQ2TMaxLimbs() const { return info_[2]; }
    std::vector<uint64_t> IndexMatrix() const {  // permuteMatrix (:110)
        std::vector<uint64_t> out((size_t)MaxSlots());
        check(he_bgv_encoder_index(h(), out.data()));
        return out;
    }
    // EncodeRingT (:203) / DecodeRingT (:341): V = std::vector<uint64_t> or std::vector<int64_t>
    template <class V> void EncodeRingT(const V &values, uint64_t scale, Poly &pT) const {
        check(he_bgv_encode_ring_t(h(), scale, up(values), values.size() / pT.Batch(), is_signed<V>(), pT.Batch(), pT.h()));
    }
    template <class V> void DecodeRingT(const Poly &pT, uint64_t scale, V &values) const {
        values.resize((size_t)pT.Batch() * MaxSlots());
        check(he_bgv_decode_ring_t(h(), scale, pT.h(), is_signed<V>(), up(values)));
    }
    // RingT2Q (:378; toP: pQ is a polynomial of ringP) / RingQ2T (:412)
    void RingT2Q(int level, bool scaleUp, const Poly &pT, Poly &pQ, bool toP = false) const {
        check(he_bgv_ring_t2q(h(), level, scaleUp, toP, pT.h(), pQ.h()));
    }
    void RingQ2T(int level, bool scaleDown, const Poly &pQ, Poly &pT) const { check(he_bgv_ring_q2t(h(), level, scaleDown, pQ.h(), pT.h())); }
    // Encode (:143), and EmbedScale (:268) into a ring.Poly: Embed (:336) is scaleUp = false
    template <class V> void Encode(const V &values, const MetaData &m, Poly &pt) const { EmbedScale(values, true, m, pt, m.IsBatched); }
    template <class V> void Embed(const V &values, const MetaData &m, Poly &polyOut) const { EmbedScale(values, false, m, polyOut); }
    template <class V> void EmbedScale(const V &values, bool scaleUp, const MetaData &m, Poly &polyOut, bool batched = true) const {
        check(he_bgv_encode(h(), polyOut.Level(), m.Scale, batched, m.IsNTT, m.IsMontgomery, scaleUp, up(values), values.size() / polyOut.Batch(),
                            is_signed<V>(), polyOut.Batch(), polyOut.h()));
    }
    // EmbedScale into a ringqp.Poly (:280-311)
    template <class V> void EncodeQP(const V &values, bool scaleUp, const MetaData &m, Poly &polyQ, Poly &polyP) const {
        check(he_bgv_encode_qp(h(), polyQ.Level(), polyP.Level(), m.Scale, m.IsNTT, m.IsMontgomery, scaleUp, up(values), values.size() / polyQ.Batch(),
                               is_signed<V>(), polyQ.Batch(), polyQ.h(), polyP.h()));
    }
    // Decode (:470)
    template <class V> void Decode(const Poly &pt, const MetaData &m, V &values) const {
        values.resize((size_t)pt.Batch() * MaxSlots());
        check(he_bgv_decode(h(), pt.Level(), m.Scale, m.IsBatched, m.IsNTT, pt.h(), is_signed<V>(), up(values)));
    }
};
}  // namespace bgv

// ---- the randomness source and the ring samplers (utils/sampling, ring/sampler_*.go; hering_sampler.h) ---------------------------
// Every sampler is an exact function of the bytes its PRNG serves: the words, the bytes consumed and the position of the source
// afterwards are the reference's.  A Poly of B entries is B successive Reads, entry 0 first.
namespace sampling {
// sampling.PRNG.  PRNG(): crypto/rand's analogue, getrandom(2).  PRNG(read): any io.Reader -- read(dst, n) fills n bytes and returns
// true (false, or an exception: a failed read, HE_EPRNG).  Position(): the bytes consumed in the reference's sense.
class PRNG {
    detail::Ref r_;
    std::shared_ptr<std::function<bool(uint8_t *, size_t)>> read_;
    static int trampoline(void *user, uint8_t *dst, size_t n) {
        try {
            return (*static_cast<std::function<bool(uint8_t *, size_t)> *>(user))(dst, n) ? 0 : 1;
        } catch (...) {
            return 2;
        }
    }

public:
    PRNG() {
        he_handle h = 0;
        check(he_prng_create_system(&h));
        r_ = detail::own(h, he_prng_destroy);
    }
    explicit PRNG(std::function<bool(uint8_t *, size_t)> read) : read_(std::make_shared<std::function<bool(uint8_t *, size_t)>>(std::move(read))) {
        he_handle h = 0;
        check(he_prng_create_callback(&PRNG::trampoline, read_.get(), &h));
        r_ = detail::own(h, he_prng_destroy);
    }
    he_handle h() const { return r_->h; }
    uint64_t Position() const {
        uint64_t v[2] = {0, 0};
        check(he_prng_position(h(), v));
        return v[0];
    }
};
}  // namespace sampling

// ring.UniformSampler (ring/sampler_uniform.go); with ringP, ringqp.UniformSampler (ring/ringqp/samplers.go) on (Q, P) pairs
class UniformSampler {
    sampling::PRNG prng_;
    Ring ring_;
    std::shared_ptr<Ring> ringP_;

public:
    UniformSampler(const sampling::PRNG &prng, const Ring &baseRing) : prng_(prng), ring_(baseRing) {}
    UniformSampler(const sampling::PRNG &prng, const Ring &ringQ, const Ring &ringP) : prng_(prng), ring_(ringQ), ringP_(std::make_shared<Ring>(ringP)) {}
    UniformSampler AtLevel(int level) const { return UniformSampler(prng_, ring_.AtLevel(level)); }
    UniformSampler AtLevel(int levelQ, int levelP) const {
        if (!ringP_) throw std::invalid_argument("UniformSampler::AtLevel(levelQ, levelP): the sampler was built over one ring");
        return UniformSampler(prng_, ring_.AtLevel(levelQ), ringP_->AtLevel(levelP));
    }
    void Read(Poly &pol) const { check(he_sampler_uniform_read(ring_.h(), ring_.Level(), 0, 0, prng_.h(), 0, pol.h(), 0)); }
    void ReadAndAdd(Poly &pol) const { check(he_sampler_uniform_read(ring_.h(), ring_.Level(), 0, 0, prng_.h(), 1, pol.h(), 0)); }
    void Read(Poly &q, Poly &p) const { check(he_sampler_uniform_read(ring_.h(), ring_.Level(), ringP_->h(), ringP_->Level(), prng_.h(), 0, q.h(), p.h())); }
    void ReadAndAdd(Poly &q, Poly &p) const { check(he_sampler_uniform_read(ring_.h(), ring_.Level(), ringP_->h(), ringP_->Level(), prng_.h(), 1, q.h(), p.h())); }
    Poly ReadNew(int batch = 1) const {
        Poly pol = ring_.NewPoly(batch);
        Read(pol);
        return pol;
    }
};
// ring.DiscreteGaussian and ring.GaussianSampler (ring/sampler_gaussian.go), the float64 branch
struct DiscreteGaussian {
    double Sigma = 3.2, Bound = 19.2;
};
class GaussianSampler {
    sampling::PRNG prng_;
    Ring ring_;
    DiscreteGaussian xe_;
    bool montgomery_;

public:
    GaussianSampler(const sampling::PRNG &prng, const Ring &baseRing, DiscreteGaussian X, bool montgomery)
        : prng_(prng), ring_(baseRing), xe_(X), montgomery_(montgomery) {}
    GaussianSampler AtLevel(int level) const { return GaussianSampler(prng_, ring_.AtLevel(level), xe_, montgomery_); }
    void Read(Poly &pol) const { check(he_sampler_gaussian_read(ring_.h(), ring_.Level(), prng_.h(), xe_.Sigma, xe_.Bound, montgomery_, 0, pol.h())); }
    void ReadAndAdd(Poly &pol) const { check(he_sampler_gaussian_read(ring_.h(), ring_.Level(), prng_.h(), xe_.Sigma, xe_.Bound, montgomery_, 1, pol.h())); }
    Poly ReadNew(int batch = 1) const {
        Poly pol = ring_.NewPoly(batch);
        Read(pol);
        return pol;
    }
};
// ring.Ternary{P} and ring.TernarySampler (ring/sampler_ternary.go); the sparse form Ternary{H} is SparseTernarySampler below
struct Ternary {
    double P = 2.0 / 3.0;
};
class TernarySampler {
    sampling::PRNG prng_;
    Ring ring_;
    Ternary xs_;
    bool montgomery_;

public:
    TernarySampler(const sampling::PRNG &prng, const Ring &baseRing, Ternary X, bool montgomery)
        : prng_(prng), ring_(baseRing), xs_(X), montgomery_(montgomery) {}
    TernarySampler AtLevel(int level) const { return TernarySampler(prng_, ring_.AtLevel(level), xs_, montgomery_); }
    void Read(Poly &pol) const { check(he_sampler_ternary_read(ring_.h(), ring_.Level(), prng_.h(), xs_.P, montgomery_, 0, pol.h())); }
    void ReadAndAdd(Poly &pol) const { check(he_sampler_ternary_read(ring_.h(), ring_.Level(), prng_.h(), xs_.P, montgomery_, 1, pol.h())); }
    Poly ReadNew(int batch = 1) const {
        Poly pol = ring_.NewPoly(batch);
        Read(pol);
        return pol;
    }
};

// ring.Ternary{H} and its TernarySampler (sampleSparse, ring/sampler_ternary.go:198-263; hering_keygen.h): Read only
class SparseTernarySampler {
    sampling::PRNG prng_;
    Ring ring_;
    int hw_;
    bool montgomery_;

public:
    SparseTernarySampler(const sampling::PRNG &prng, const Ring &baseRing, int H, bool montgomery)
        : prng_(prng), ring_(baseRing), hw_(H), montgomery_(montgomery) {}
    SparseTernarySampler AtLevel(int level) const { return SparseTernarySampler(prng_, ring_.AtLevel(level), hw_, montgomery_); }
    void Read(Poly &pol) const { check(he_keygen_ternary_sparse_read(ring_.h(), ring_.Level(), prng_.h(), hw_, montgomery_, pol.h())); }
};

// ---- rlwe.Encryptor / rlwe.Decryptor / KeyGenerator.GenPublicKey (core/rlwe/encryptor.go, decryptor.go, keygenerator.go:80-88;
// hering_encryptor.h).  Every call is an exact function of the bytes the encryptor's PRNG serves; for a batch the draws are made step
// by step over the entries.  Keys carry the batch of the ciphertexts.
namespace rlwe {
// ringqp.Poly: a (Q, P) pair
struct PolyQP {
    Poly Q, P;
};
// rlwe.SecretKey: Value in the NTT domain and Montgomery form
struct SecretKey {
    PolyQP Value;
};
// rlwe.PublicKey: Value[0], Value[1], NTT and Montgomery
struct PublicKey {
    std::array<PolyQP, 2> Value;
};
// rlwe.MetaData restricted to what the encryptor and the decryptor read
struct MetaData {
    bool IsNTT = true, IsMontgomery = false;
};
// rlwe.Plaintext / rlwe.Ciphertext (Element[ring.Poly]): level = limbs in use - 1 (Resize changes it, not the storage)
struct Plaintext {
    Poly Value;
    MetaData Meta;
    int level = -1;
    int Level() const { return level < 0 ? Value.Level() : level; }
};
struct Ciphertext {
    std::vector<Poly> Value;
    MetaData Meta;
    int level = -1;
    int Level() const { return level < 0 ? Value[0].Level() : level; }
    int Degree() const { return (int)Value.size() - 1; }
};
// rlwe.Element[ringqp.Poly] of degree 1
struct ElementQP {
    std::array<PolyQP, 2> Value;
    MetaData Meta{true, true};
    int LevelQ() const { return Value[0].Q.Level(); }
    int LevelP() const { return Value[0].P.Level(); }
};

class Encryptor {
    detail::Ref r_;
    Evaluator eval_;
    sampling::PRNG prng_;
    Ternary xs_;
    DiscreteGaussian xe_;
    std::vector<Poly> key_;  // what keeps the bound key alive
    void bind(int kind, std::vector<Poly> key) {
        he_handle k[4] = {0, 0, 0, 0};
        for (size_t i = 0; i < key.size() && i < 4; i++) k[i] = key[i].h();
        check(he_encryptor_set_key(r_->h, kind, k));
        key_ = std::move(key);
    }

public:
    // rlwe.NewEncryptor(params, nil)
    Encryptor(const Evaluator &eval, const sampling::PRNG &prng, Ternary Xs = {}, DiscreteGaussian Xe = {}) : eval_(eval), prng_(prng), xs_(Xs), xe_(Xe) {
        he_handle h = 0;
        check(he_encryptor_create(eval.h(), prng.h(), Xs.P, Xe.Sigma, Xe.Bound, &h));
        r_ = detail::own(h, he_encryptor_destroy);
    }
    he_handle h() const { return r_->h; }
    // WithKey: a shallow copy bound to the key
    Encryptor WithKey(const SecretKey &sk) const {
        Encryptor e(eval_, prng_, xs_, xe_);
        e.bind(1, {sk.Value.Q, sk.Value.P});
        return e;
    }
    Encryptor WithKey(const PublicKey &pk) const {
        Encryptor e(eval_, prng_, xs_, xe_);
        e.bind(2, {pk.Value[0].Q, pk.Value[0].P, pk.Value[1].Q, pk.Value[1].P});
        return e;
    }
    void EncryptZero(Ciphertext &ct) const { check(he_encrypt_zero(h(), ct.Level(), ct.Meta.IsNTT, ct.Meta.IsMontgomery, ct.Value[0].h(), ct.Value[1].h())); }
    void EncryptZero(ElementQP &ct) const {
        check(he_encrypt_zero_qp(h(), ct.LevelQ(), ct.Value[0].P.h() ? ct.LevelP() : -1, ct.Meta.IsNTT, ct.Meta.IsMontgomery, ct.Value[0].Q.h(),
                                 ct.Value[0].P.h(), ct.Value[1].Q.h(), ct.Value[1].P.h()));
    }
    // Encrypt (:134-152): the ciphertext takes the plaintext's metadata and level = min of the two
    void Encrypt(const Plaintext &pt, Ciphertext &ct) const {
        int level = 0;
        check(he_encrypt(h(), pt.Level(), ct.Level(), pt.Meta.IsNTT, pt.Meta.IsMontgomery, pt.Value.h(), ct.Value[0].h(), ct.Value[1].h(), &level));
        ct.Meta = pt.Meta;
        ct.level = level;
    }
    void addPtToCt(int level, const Plaintext &pt, Ciphertext &ct) const {
        check(he_add_pt_to_ct(h(), level, pt.Meta.IsNTT, ct.Meta.IsNTT, pt.Value.h(), ct.Value[0].h()));
    }
};

class Decryptor {
    detail::Ref r_;
    SecretKey sk_;

public:
    // rlwe.NewDecryptor(params, sk)
    Decryptor(const Evaluator &eval, const SecretKey &sk) : sk_(sk) {
        he_handle h = 0;
        check(he_decryptor_create(eval.h(), sk.Value.Q.h(), &h));
        r_ = detail::own(h, he_decryptor_destroy);
    }
    // Decrypt (:51-93): pt takes the ciphertext's metadata and level = min of the two
    void Decrypt(const Ciphertext &ct, Plaintext &pt) const {
        std::vector<he_handle> hs;
        for (const Poly &p : ct.Value) hs.push_back(p.h());
        int level = 0;
        check(he_decryptor_decrypt(r_->h, ct.Level(), pt.Level(), ct.Meta.IsNTT, ct.Degree(), hs.data(), pt.Value.h(), &level));
        pt.Meta = ct.Meta;
        pt.level = level;
    }
};

// rlwe.EvaluationKeyParameters (core/rlwe/evaluationkey.go): a negative level = the parameters' default; Compressed keys are not built
struct EvaluationKeyParameters {
    int LevelQ = -2, LevelP = -2, BaseTwoDecomposition = 0;
    bool Compressed = false;
};
// rlwe.GaloisKey
struct GaloisKey {
    EvaluationKey Key;
    uint64_t GaloisElement = 0, NthRoot = 0;
};
// AddPolyTimesGadgetVectorToGadgetCiphertext (core/rlwe/gadgetciphertext.go:172-241): pt times the gadget vector to component u of cts[u]
inline void AddPolyTimesGadgetVectorToGadgetCiphertext(const Poly &pt, const std::vector<EvaluationKey> &cts) {
    if (cts.empty() || cts.size() > 2) throw std::invalid_argument("cannot AddPolyTimesGadgetVectorToGadgetCiphertext: len(cts) should be <= 2");
    check(he_gadget_add_poly(pt.h(), cts[0].h(), cts.size() > 1 ? cts[1].h() : 0));
}

// rlwe.KeyGenerator (core/rlwe/keygenerator.go; hering_keygen.h): every call is an exact function of the bytes the generator's PRNG
// serves -- an evaluation key row after row (the uniform c1, then the Gaussian e), Galois keys key after key
class KeyGenerator {
    Encryptor enc_;
    Evaluator eval_;
    detail::Ref r_;
    static int logq(uint64_t q) {  // LogQi (params.go:474-481): round(log2(q))
        int b = 63 - __builtin_clzll(q);
        const long double m = (long double)q / (long double)((uint64_t)1 << b);  // in [1, 2): rounds up from sqrt(2)
        return m * m >= 2.0L ? b + 1 : b;
    }
    bool hasP() const { return eval_.RingP().MaxLevel() >= 0; }
    uint64_t nthRoot() const { return (uint64_t)eval_.RingQ().N() * (eval_.RingQ().Type() == RingType::Standard ? 2 : 4); }
    SecretKey newSecretKey() const { return hasP() ? SecretKey{{eval_.RingQ().NewPoly(), eval_.RingP().NewPoly()}} : SecretKey{{eval_.RingQ().NewPoly(), Poly()}}; }

public:
    KeyGenerator(const Evaluator &eval, const sampling::PRNG &prng, Ternary Xs = {}, DiscreteGaussian Xe = {}) : enc_(eval, prng, Xs, Xe), eval_(eval) {
        he_handle h = 0;
        check(he_keygen_create(eval.h(), prng.h(), Xs.P, Xe.Sigma, Xe.Bound, &h));
        r_ = detail::own(h, he_keygen_destroy);
    }
    he_handle h() const { return r_->h; }
    const Evaluator &GetEvaluator() const { return eval_; }
    // -- secret and public keys
    void GenSecretKey(SecretKey &sk) const {
        check(he_keygen_secret_key(h(), sk.Value.Q.Level(), sk.Value.P.h() ? sk.Value.P.Level() : -1, sk.Value.Q.h(), sk.Value.P.h()));
    }
    SecretKey GenSecretKeyNew() const {
        SecretKey sk = newSecretKey();
        GenSecretKey(sk);
        return sk;
    }
    void GenSecretKeyWithHammingWeight(int hw, SecretKey &sk) const {
        check(he_keygen_secret_key_hw(h(), hw, sk.Value.Q.Level(), sk.Value.P.h() ? sk.Value.P.Level() : -1, sk.Value.Q.h(), sk.Value.P.h()));
    }
    SecretKey GenSecretKeyWithHammingWeightNew(int hw) const {
        SecretKey sk = newSecretKey();
        GenSecretKeyWithHammingWeight(hw, sk);
        return sk;
    }
    void GenPublicKey(const SecretKey &sk, PublicKey &pk) const {
        ElementQP el{pk.Value, MetaData{true, true}};
        enc_.WithKey(sk).EncryptZero(el);
        pk.Value = el.Value;
    }
    PublicKey GenPublicKeyNew(const SecretKey &sk) const {
        const Ring &q = eval_.RingQ(), &p = eval_.RingP();
        PublicKey pk{{{{q.NewPoly(), hasP() ? p.NewPoly() : Poly()}, {q.NewPoly(), hasP() ? p.NewPoly() : Poly()}}}};
        GenPublicKey(sk, pk);
        return pk;
    }
    std::pair<SecretKey, PublicKey> GenKeyPairNew() const {
        SecretKey sk = GenSecretKeyNew();
        PublicKey pk = GenPublicKeyNew(sk);
        return {sk, pk};
    }
    // -- evaluation keys.  newEvaluationKey: a zeroed key of degree 1 at the resolved levels (ResolveEvaluationKeyParameters)
    EvaluationKey NewEvaluationKey(const EvaluationKeyParameters &evkParams = {}) const {
        if (evkParams.Compressed) throw std::invalid_argument("compressed evaluation keys are not on the device (hering_keygen.h)");
        const int levelQ = evkParams.LevelQ < -1 ? eval_.RingQ().MaxLevel() : evkParams.LevelQ;
        const int levelP = evkParams.LevelP < -1 ? (hasP() ? eval_.RingP().MaxLevel() : -1) : evkParams.LevelP;
        const int pw2 = evkParams.BaseTwoDecomposition;
        const int beta = levelP == -1 ? levelQ + 1 : (levelQ + levelP + 1) / (levelP + 1);  // params.go:543-550
        if (!pw2) return eval_.NewEvaluationKeyZero(beta, levelQ + 1, levelP + 1);
        std::vector<int> nj;  // BaseTwoDecompositionVectorSize (params.go:523-540)
        for (int i = 0; i < beta; i++) nj.push_back(levelP > 0 ? 1 : (logq(eval_.RingQ().ModuliChain()[(size_t)i]) + pw2 - 1) / pw2);
        int rows = 0;
        for (int n : nj) rows += n;
        return eval_.NewEvaluationKeyZero(rows, levelQ + 1, levelP + 1, pw2, nj);
    }
    // GenEvaluationKey (:261-285): the two keys may live in rings of a smaller degree and at other levels; their Q parts are read
    void GenEvaluationKey(const SecretKey &skInput, const SecretKey &skOutput, EvaluationKey &evk) const {
        check(he_keygen_evaluation_key_sk(h(), skInput.Value.Q.h(), skOutput.Value.Q.h(), evk.h()));
    }
    EvaluationKey GenEvaluationKeyNew(const SecretKey &skInput, const SecretKey &skOutput, const EvaluationKeyParameters &evkParams = {}) const {
        EvaluationKey evk = NewEvaluationKey(evkParams);
        GenEvaluationKey(skInput, skOutput, evk);
        return evk;
    }
    // genEvaluationKey (:287-330) on operands of the key's own ring and levels: the fused entry
    void genEvaluationKey(const Poly &skIn, const SecretKey &skOut, EvaluationKey &evk) const {
        check(he_keygen_evaluation_key(h(), skIn.h(), skOut.Value.Q.h(), skOut.Value.P.h(), evk.h()));
    }
    // GenEvaluationKeysForRingSwapNew (:211-233): (stdToci, ciToStd)
    std::pair<EvaluationKey, EvaluationKey> GenEvaluationKeysForRingSwapNew(const SecretKey &skStd, const SecretKey &skConjugateInvariant,
                                                                            const EvaluationKeyParameters &evkParams = {}) const {
        const int levelQ = skStd.Value.Q.Level() < skConjugateInvariant.Value.Q.Level() ? skStd.Value.Q.Level() : skConjugateInvariant.Value.Q.Level();
        SecretKey mapped{{eval_.RingQ().AtLevel(levelQ).NewPoly(), Poly()}};
        eval_.RingQ().AtLevel(levelQ).UnfoldConjugateInvariantToStandard(skConjugateInvariant.Value.Q, mapped.Value.Q);
        EvaluationKey stdToci = GenEvaluationKeyNew(skStd, mapped, evkParams);
        EvaluationKey ciToStd = GenEvaluationKeyNew(mapped, skStd, evkParams);
        return {stdToci, ciToStd};
    }
    void GenRelinearizationKey(const SecretKey &sk, EvaluationKey &rlk) const {
        check(he_keygen_relinearization_key(h(), sk.Value.Q.h(), sk.Value.P.h(), rlk.h()));
    }
    EvaluationKey GenRelinearizationKeyNew(const SecretKey &sk, const EvaluationKeyParameters &evkParams = {}) const {
        EvaluationKey rlk = NewEvaluationKey(evkParams);
        GenRelinearizationKey(sk, rlk);
        return rlk;
    }
    void GenGaloisKey(uint64_t galEl, const SecretKey &sk, GaloisKey &gk) const {
        check(he_keygen_galois_key(h(), galEl, sk.Value.Q.h(), sk.Value.P.h(), gk.Key.h()));
        gk.GaloisElement = galEl;
        gk.NthRoot = nthRoot();
    }
    GaloisKey GenGaloisKeyNew(uint64_t galEl, const SecretKey &sk, const EvaluationKeyParameters &evkParams = {}) const {
        GaloisKey gk{NewEvaluationKey(evkParams), galEl, nthRoot()};
        GenGaloisKey(galEl, sk, gk);
        return gk;
    }
    void GenGaloisKeys(const std::vector<uint64_t> &galEls, const SecretKey &sk, std::vector<GaloisKey> &gks) const {
        if (galEls.size() != gks.size()) throw std::invalid_argument("galEls and gks must have the same length");
        std::vector<he_handle> hs;
        for (GaloisKey &gk : gks) {
            if (!gk.Key.h()) gk.Key = NewEvaluationKey();
            hs.push_back(gk.Key.h());
        }
        check(he_keygen_galois_keys(h(), (int)galEls.size(), galEls.data(), sk.Value.Q.h(), sk.Value.P.h(), hs.data()));
        for (size_t i = 0; i < gks.size(); i++) {
            gks[i].GaloisElement = galEls[i];
            gks[i].NthRoot = nthRoot();
        }
    }
    std::vector<GaloisKey> GenGaloisKeysNew(const std::vector<uint64_t> &galEls, const SecretKey &sk, const EvaluationKeyParameters &evkParams = {}) const {
        std::vector<GaloisKey> gks;
        for (uint64_t g : galEls) gks.push_back(GaloisKey{NewEvaluationKey(evkParams), g, nthRoot()});
        GenGaloisKeys(galEls, sk, gks);
        return gks;
    }
};
}  // namespace rlwe
using KeyGenerator = rlwe::KeyGenerator;

// The threshold protocols of the reference's multiparty package (hering_multiparty.h), with the reference's method names and argument
// order.  A protocol object is one party's view: its private samplers are its rlwe::KeyGenerator, the common reference string any
// sampling::PRNG.  Gadget-shaped CRPs and shares live in EvaluationKey handles: a CRP in component 1, a degree-0 share in component
// 0, a round-one share of the relinearization protocol in both.  A Go error is an exception (hering::Error, std::invalid_argument).
namespace multiparty {
using CRS = sampling::PRNG;
// EvaluationKeyGenCRP / EvaluationKeyGenShare / RelinearizationKeyGenShare: Degree = the components in use, minus one
struct GadgetShare {
    EvaluationKey Key;
    int Degree = 0;
};
using EvaluationKeyGenCRP = GadgetShare;
using EvaluationKeyGenShare = GadgetShare;
using RelinearizationKeyGenCRP = GadgetShare;
using RelinearizationKeyGenShare = GadgetShare;
struct GaloisKeyGenShare : GadgetShare {
    uint64_t GaloisElement = 0;
};
using GaloisKeyGenCRP = GadgetShare;

class EvaluationKeyGenProtocol {
protected:
    rlwe::KeyGenerator kgen_;

public:
    explicit EvaluationKeyGenProtocol(const rlwe::KeyGenerator &kgen) : kgen_(kgen) {}
    EvaluationKeyGenShare AllocateShare(const rlwe::EvaluationKeyParameters &evkParams = {}) const { return {kgen_.NewEvaluationKey(evkParams), 0}; }
    // sampleCRP (keygen_evk.go:64-83): i outer and j inner, one ringqp uniform ReadNew per row
    EvaluationKeyGenCRP SampleCRP(const CRS &crs, const rlwe::EvaluationKeyParameters &evkParams = {}) const {
        GadgetShare crp{kgen_.NewEvaluationKey(evkParams), 0};
        check(he_mp_crp_gadget(kgen_.GetEvaluator().h(), crs.h(), crp.Key.h()));
        return crp;
    }
    void GenShare(const rlwe::SecretKey &skIn, const rlwe::SecretKey &skOut, const EvaluationKeyGenCRP &crp, EvaluationKeyGenShare &shareOut) const {
        check(he_mp_evk_gen_share(kgen_.h(), skIn.Value.Q.h(), skOut.Value.Q.h(), skOut.Value.P.h(), crp.Key.h(), shareOut.Key.h()));
        shareOut.Degree = 0;
    }
    // one Add per word on components 0..Degree()
    void AggregateShares(const GadgetShare &share1, const GadgetShare &share2, GadgetShare &share3) const {
        check(he_mp_gadget_aggregate(share1.Key.h(), share2.Key.h(), share1.Degree, share3.Key.h()));
        share3.Degree = share1.Degree;
    }
    void GenEvaluationKey(const EvaluationKeyGenShare &share, const EvaluationKeyGenCRP &crp, EvaluationKey &evk) const {
        check(he_mp_evk_finalize(share.Key.h(), crp.Key.h(), evk.h()));
    }
};

class GaloisKeyGenProtocol : public EvaluationKeyGenProtocol {
public:
    using EvaluationKeyGenProtocol::EvaluationKeyGenProtocol;
    GaloisKeyGenShare AllocateShare(const rlwe::EvaluationKeyParameters &evkParams = {}) const {
        GaloisKeyGenShare s;
        s.Key = kgen_.NewEvaluationKey(evkParams);
        return s;
    }
    void GenShare(const rlwe::SecretKey &sk, uint64_t galEl, const GaloisKeyGenCRP &crp, GaloisKeyGenShare &shareOut) const {
        check(he_mp_galois_gen_share(kgen_.h(), galEl, sk.Value.Q.h(), sk.Value.P.h(), crp.Key.h(), shareOut.Key.h()));
        shareOut.GaloisElement = galEl;  // "Important" (keygen_gal.go:60)
        shareOut.Degree = 0;
    }
    void AggregateShares(const GaloisKeyGenShare &share1, const GaloisKeyGenShare &share2, GaloisKeyGenShare &share3) const {
        if (share1.GaloisElement != share2.GaloisElement)
            throw std::invalid_argument("cannot aggregate: GaloisKeyGenShares do not share the same GaloisElement");
        share3.GaloisElement = share1.GaloisElement;
        EvaluationKeyGenProtocol::AggregateShares(share1, share2, share3);
    }
    void GenGaloisKey(const GaloisKeyGenShare &share, const GaloisKeyGenCRP &crp, rlwe::GaloisKey &gk) const {
        GenEvaluationKey(share, crp, gk.Key);
        const Ring &q = kgen_.GetEvaluator().RingQ();
        gk.GaloisElement = share.GaloisElement;
        gk.NthRoot = (uint64_t)q.N() * (q.Type() == RingType::Standard ? 2 : 4);
    }
};

class RelinearizationKeyGenProtocol : public EvaluationKeyGenProtocol {
public:
    using EvaluationKeyGenProtocol::EvaluationKeyGenProtocol;
    struct Shares {
        rlwe::SecretKey ephSk;
        RelinearizationKeyGenShare r1, r2;
    };
    // (ephSk at the parameters' top levels, a degree-1 and a degree-0 share)
    Shares AllocateShare(const rlwe::EvaluationKeyParameters &evkParams = {}) const {
        const Evaluator &ev = kgen_.GetEvaluator();
        const bool hasP = ev.RingP().MaxLevel() >= 0;
        return {rlwe::SecretKey{{ev.RingQ().NewPoly(), hasP ? ev.RingP().NewPoly() : Poly()}}, {kgen_.NewEvaluationKey(evkParams), 1},
                {kgen_.NewEvaluationKey(evkParams), 0}};
    }
    void GenShareRoundOne(const rlwe::SecretKey &sk, const RelinearizationKeyGenCRP &crp, rlwe::SecretKey &ephSkOut, RelinearizationKeyGenShare &shareOut) const {
        check(he_mp_rkg_round_one(kgen_.h(), sk.Value.Q.h(), sk.Value.P.h(), crp.Key.h(), ephSkOut.Value.Q.h(), ephSkOut.Value.P.h(), shareOut.Key.h()));
        shareOut.Degree = 1;
    }
    // words in [0, 2q), as the reference leaves them
    void GenShareRoundTwo(const rlwe::SecretKey &ephSk, const rlwe::SecretKey &sk, const RelinearizationKeyGenShare &round1,
                          RelinearizationKeyGenShare &shareOut) const {
        check(he_mp_rkg_round_two(kgen_.h(), ephSk.Value.Q.h(), ephSk.Value.P.h(), sk.Value.Q.h(), sk.Value.P.h(), round1.Key.h(), shareOut.Key.h()));
        shareOut.Degree = 0;
    }
    void GenRelinearizationKey(const RelinearizationKeyGenShare &round1, const RelinearizationKeyGenShare &round2, EvaluationKey &evalKeyOut) const {
        check(he_mp_rlk_finalize(round1.Key.h(), round2.Key.h(), evalKeyOut.h()));
    }
};

using PublicKeyGenCRP = rlwe::PolyQP;
using PublicKeyGenShare = rlwe::PolyQP;
class PublicKeyGenProtocol {
    rlwe::KeyGenerator kgen_;
    bool hasP() const { return kgen_.GetEvaluator().RingP().MaxLevel() >= 0; }

public:
    explicit PublicKeyGenProtocol(const rlwe::KeyGenerator &kgen) : kgen_(kgen) {}
    PublicKeyGenShare AllocateShare() const {
        const Evaluator &ev = kgen_.GetEvaluator();
        return {ev.RingQ().NewPoly(), hasP() ? ev.RingP().NewPoly() : Poly()};
    }
    PublicKeyGenCRP SampleCRP(const CRS &crs) const {
        const Evaluator &ev = kgen_.GetEvaluator();
        PublicKeyGenCRP crp = AllocateShare();
        if (hasP()) UniformSampler(crs, ev.RingQ(), ev.RingP()).Read(crp.Q, crp.P);
        else UniformSampler(crs, ev.RingQ()).Read(crp.Q);
        return crp;
    }
    void GenShare(const rlwe::SecretKey &sk, const PublicKeyGenCRP &crp, PublicKeyGenShare &shareOut) const {
        check(he_mp_pk_gen_share(kgen_.h(), sk.Value.Q.h(), sk.Value.P.h(), crp.Q.h(), crp.P.h(), shareOut.Q.h(), shareOut.P.h()));
    }
    void AggregateShares(const PublicKeyGenShare &share1, const PublicKeyGenShare &share2, PublicKeyGenShare &shareOut) const {
        const Evaluator &ev = kgen_.GetEvaluator();
        ev.RingQ().Add(share1.Q, share2.Q, shareOut.Q);
        if (hasP()) ev.RingP().Add(share1.P, share2.P, shareOut.P);
    }
    void GenPublicKey(const PublicKeyGenShare &roundShare, const PublicKeyGenCRP &crp, rlwe::PublicKey &pubkey) const {
        const rlwe::PolyQP *src[2] = {&roundShare, &crp};
        for (int k = 0; k < 2; k++) {
            pubkey.Value[(size_t)k].Q.CopyLvl(src[k]->Q.Level(), src[k]->Q);
            if (hasP()) pubkey.Value[(size_t)k].P.CopyLvl(src[k]->P.Level(), src[k]->P);
        }
    }
};

// NewKeySwitchProtocol / NewPublicKeySwitchProtocol: DiscreteGaussian{sqrt(NoiseFreshSK^2 + noise.Sigma^2), 6 sigma} (keyswitch_sk.go:49-52)
inline DiscreteGaussian SmudgingNoise(double noiseSigma, double NoiseFreshSK) {
    const double s = std::sqrt(NoiseFreshSK * NoiseFreshSK + noiseSigma * noiseSigma);
    return DiscreteGaussian{s, 6 * s};
}
struct KeySwitchCRP {
    Poly Value;
};
struct KeySwitchShare {
    Poly Value;  // words in [0, 2q)
    int Level() const { return Value.Level(); }
};
class KeySwitchProtocol {
    rlwe::KeyGenerator kgen_;
    DiscreteGaussian noise_;

public:
    // (kgen, noiseFlooding.Sigma, the parameters' NoiseFreshSK)
    KeySwitchProtocol(const rlwe::KeyGenerator &kgen, double noiseSigma, double NoiseFreshSK) : kgen_(kgen), noise_(SmudgingNoise(noiseSigma, NoiseFreshSK)) {}
    const DiscreteGaussian &Noise() const { return noise_; }
    KeySwitchShare AllocateShare(int level) const { return {kgen_.GetEvaluator().RingQ().AtLevel(level).NewPoly()}; }
    KeySwitchCRP SampleCRP(int level, const CRS &crs) const { return {UniformSampler(crs, kgen_.GetEvaluator().RingQ().AtLevel(level)).ReadNew()}; }
    void GenShare(const rlwe::SecretKey &skInput, const rlwe::SecretKey &skOutput, const rlwe::Ciphertext &ct, KeySwitchShare &shareOut) const {
        const int level = shareOut.Level() < ct.Value[1].Level() ? shareOut.Level() : ct.Value[1].Level();  // :84
        check(he_mp_cks_gen_share(kgen_.h(), level, skInput.Value.Q.h(), skOutput.Value.Q.h(), ct.Value[1].h(), ct.Meta.IsNTT, noise_.Sigma, noise_.Bound,
                                  shareOut.Value.h()));
    }
    void AggregateShares(const KeySwitchShare &share1, const KeySwitchShare &share2, KeySwitchShare &shareOut) const {
        if (share1.Level() != share2.Level() || share1.Level() != shareOut.Level()) throw std::invalid_argument("cannot AggregateShares: shares levels do not match");
        kgen_.GetEvaluator().RingQ().AtLevel(share1.Level()).Add(share1.Value, share2.Value, shareOut.Value);
    }
    void KeySwitch(const rlwe::Ciphertext &ctIn, const KeySwitchShare &combined, rlwe::Ciphertext &opOut) const {
        const int level = ctIn.Level();
        if (&ctIn != &opOut) {
            opOut.Value[1].CopyLvl(level, ctIn.Value[1]);
            opOut.Meta = ctIn.Meta;
            opOut.level = level;
        }
        kgen_.GetEvaluator().RingQ().AtLevel(level).Add(ctIn.Value[0], combined.Value, opOut.Value[0]);
    }
};

using PublicKeySwitchShare = rlwe::Ciphertext;
class PublicKeySwitchProtocol {
    rlwe::Encryptor enc_;
    Evaluator eval_;
    sampling::PRNG noisePrng_;
    DiscreteGaussian noise_;

public:
    // (the party's encryptor with its own source, its evaluator, the source of the smudging noise, noiseFlooding.Sigma, NoiseFreshSK)
    PublicKeySwitchProtocol(const rlwe::Encryptor &enc, const Evaluator &eval, const sampling::PRNG &noisePrng, double noiseSigma, double NoiseFreshSK)
        : enc_(enc), eval_(eval), noisePrng_(noisePrng), noise_(SmudgingNoise(noiseSigma, NoiseFreshSK)) {}
    PublicKeySwitchShare AllocateShare(int levelQ) const {
        const Ring r = eval_.RingQ().AtLevel(levelQ);
        return rlwe::Ciphertext{{r.NewPoly(), r.NewPoly()}, rlwe::MetaData{}, -1};
    }
    void GenShare(const rlwe::SecretKey &sk, const rlwe::PublicKey &pk, const rlwe::Ciphertext &ct, PublicKeySwitchShare &shareOut) const {
        const int level = shareOut.Value[0].Level() < ct.Value[1].Level() ? shareOut.Value[0].Level() : ct.Value[1].Level();  // :71
        const rlwe::Encryptor enc = enc_.WithKey(pk);
        check(he_mp_pcks_gen_share(enc.h(), noisePrng_.h(), level, sk.Value.Q.h(), ct.Value[1].h(), ct.Meta.IsNTT, ct.Meta.IsMontgomery, noise_.Sigma,
                                   noise_.Bound, shareOut.Value[0].h(), shareOut.Value[1].h()));
        shareOut.Meta = ct.Meta;
    }
    void AggregateShares(const PublicKeySwitchShare &share1, const PublicKeySwitchShare &share2, PublicKeySwitchShare &shareOut) const {
        if (share1.Value[0].Level() != share1.Value[1].Level()) throw std::invalid_argument("cannot AggregateShares: the two shares are at different levelQ");
        const Ring r = eval_.RingQ().AtLevel(share1.Value[0].Level());
        for (size_t k = 0; k < 2; k++) r.Add(share1.Value[k], share2.Value[k], shareOut.Value[k]);
    }
    void KeySwitch(const rlwe::Ciphertext &ctIn, const PublicKeySwitchShare &combined, rlwe::Ciphertext &opOut) const {
        const int level = ctIn.Level();
        if (&ctIn != &opOut) {
            opOut.Meta = ctIn.Meta;
            opOut.level = level;
        }
        eval_.RingQ().AtLevel(level).Add(ctIn.Value[0], combined.Value[0], opOut.Value[0]);
        opOut.Value[1].CopyLvl(level, combined.Value[1]);
    }
};
}  // namespace multiparty

// ---- RGSW (core/rgsw; hering_rgsw.h), NTT domain -----------------------------------------------------------------------------
namespace rgsw {
// rgsw.Ciphertext (core/rgsw/elements.go:12): Value [2]rlwe.GadgetCiphertext, two device keys of one evaluator and one shape
struct Ciphertext {
    std::array<EvaluationKey, 2> Value;
    int LevelQ() const { return Value[0].LevelQ(); }
    int LevelP() const { return Value[0].LevelP(); }
};
// rgsw.Evaluator (core/rgsw/evaluator.go:14): an rlwe.Evaluator with the external product
class Evaluator : public hering::Evaluator {
public:
    using hering::Evaluator::Evaluator;
    explicit Evaluator(const hering::Evaluator &ev) : hering::Evaluator(ev) {}
    // ExternalProduct (:39): opOut = (<op0, op1[0]>, <op0, op1[1]>) at the levels of op1; opOut may be op0
    void ExternalProduct(const hering::Ciphertext &op0, const Ciphertext &op1, hering::Ciphertext &opOut) const {
        check(he_rgsw_external_product(h(), op0.Value.at(0).h(), op0.Value.at(1).h(), op1.Value[0].h(), op1.Value[1].h(),
                                       opOut.Value.at(0).h(), opOut.Value.at(1).h()));
    }
    // batch entry b of op0 times key sel[b] of a resident key table (he_rgsw_keyset_create); sel[b] == -1 passes the entry through
    void ExternalProductSelect(const hering::Ciphertext &op0, he_handle keySet, const std::vector<int32_t> &sel, hering::Ciphertext &opOut) const {
        check(he_rgsw_external_product_select(h(), op0.Value.at(0).h(), op0.Value.at(1).h(), keySet, sel.data(), (int)sel.size(),
                                              opOut.Value.at(0).h(), opOut.Value.at(1).h()));
    }
};
// rgsw.NewCiphertext (elements.go:27): a zeroed ciphertext at the levels and BaseTwoDecomposition of evkParams
inline Ciphertext NewCiphertext(const rlwe::KeyGenerator &kgen, const rlwe::EvaluationKeyParameters &evkParams = {}) {
    return Ciphertext{{kgen.NewEvaluationKey(evkParams), kgen.NewEvaluationKey(evkParams)}};
}
// rgsw.Encryptor (core/rgsw/encryptor.go; hering_rgsw_encryptor.h): an rlwe.Encryptor under a secret key whose Encrypt and
// EncryptZero also take an rgsw.Ciphertext.  Every call is an exact function of the bytes the PRNG serves; per row (i, j) one
// encryptZeroSk on Value[0][i][j], then one on Value[1][i][j]; in a table, ciphertext after ciphertext.
class Encryptor {
    rlwe::Encryptor enc_;

public:
    // rgsw.NewEncryptor(params, key): only secret-key encryption is supported
    Encryptor(const hering::Evaluator &params, const sampling::PRNG &prng, const rlwe::SecretKey &key, DiscreteGaussian Xe = {})
        : enc_(rlwe::Encryptor(params, prng, Ternary{}, Xe).WithKey(key)) {}
    he_handle h() const { return enc_.h(); }
    void EncryptZero(Ciphertext &ct) const { check(he_rgsw_encrypt_zero(h(), ct.Value[0].h(), ct.Value[1].h())); }
    // Encrypt (:25-73): EncryptZero, then pt times the gadget vector to component 0 of Value[0] and component 1 of Value[1]
    void Encrypt(const rlwe::Plaintext &pt, Ciphertext &ct) const {
        check(he_rgsw_encrypt(h(), pt.Value.h(), pt.Meta.IsNTT, pt.Meta.IsMontgomery, ct.Value[0].h(), ct.Value[1].h()));
    }
    // operands that are no RGSW ciphertexts go to the embedded rlwe.Encryptor
    void EncryptZero(rlwe::Ciphertext &ct) const { enc_.EncryptZero(ct); }
    void EncryptZero(rlwe::ElementQP &ct) const { enc_.EncryptZero(ct); }
    void Encrypt(const rlwe::Plaintext &pt, rlwe::Ciphertext &ct) const { enc_.Encrypt(pt, ct); }
    // cts[k] = Encrypt(entry sel[k] of pts) on the one source, ciphertext 0 first; pts: batch entries, NTT and Montgomery (an empty
    // Poly when every sel is -1); sel[k] == -1: EncryptZero
    void EncryptTable(const Poly &pts, const std::vector<int32_t> &sel, std::vector<Ciphertext> &cts) const {
        if (sel.size() != cts.size()) throw std::invalid_argument("EncryptTable: one selection per ciphertext");
        std::vector<he_handle> k0, k1;
        for (const Ciphertext &c : cts) { k0.push_back(c.Value[0].h()); k1.push_back(c.Value[1].h()); }
        check(he_rgsw_encrypt_table(h(), pts.h(), sel.data(), (int)cts.size(), k0.data(), k1.data()));
    }
};
}  // namespace rgsw

// ---- blind rotation (core/rgsw/blindrot; hering_blindrot.h), NTT domain ---------------------------------------------------------
// The device entries only: Evaluate's prologue (the switch to modulus 2N and the accumulators' initial values) is the caller's.
namespace blindrot {
// a table of RGSW ciphertexts resident on the device (BlindRotationEvaluationKeySet's blind rotation keys)
class RGSWKeySet {
    detail::Ref r_;
    std::vector<rgsw::Ciphertext> keys_;

public:
    RGSWKeySet(const hering::Evaluator &ev, const std::vector<rgsw::Ciphertext> &keys) : keys_(keys) {
        std::vector<he_handle> k0, k1;
        for (const rgsw::Ciphertext &k : keys) { k0.push_back(k.Value[0].h()); k1.push_back(k.Value[1].h()); }
        he_handle h = 0;
        check(he_rgsw_keyset_create(ev.h(), (int)keys.size(), k0.data(), k1.data(), &h));
        r_ = detail::own(h, he_rgsw_keyset_destroy);
    }
    he_handle h() const { return r_->h; }
    size_t size() const { return keys_.size(); }
    const std::vector<rgsw::Ciphertext> &Keys() const { return keys_; }
};
// the Galois keys of a blind rotation with their Galois elements and index tables (GetEvaluationKeySet, keys.go:41)
class GaloisKeySet {
    detail::Ref r_;
    std::vector<uint64_t> galEls_;
    std::vector<EvaluationKey> keys_;

public:
    GaloisKeySet(const hering::Evaluator &ev, const std::vector<uint64_t> &galEls, const std::vector<EvaluationKey> &keys) : galEls_(galEls), keys_(keys) {
        if (galEls.size() != keys.size()) throw std::invalid_argument("GaloisKeySet: one Galois element per key");
        std::vector<he_handle> k;
        for (const EvaluationKey &e : keys) k.push_back(e.h());
        he_handle h = 0;
        check(he_galois_keyset_create(ev.h(), (int)keys.size(), galEls.data(), k.data(), &h));
        r_ = detail::own(h, he_galois_keyset_destroy);
    }
    he_handle h() const { return r_->h; }
    const std::vector<uint64_t> &GaloisElements() const { return galEls_; }
    const std::vector<EvaluationKey> &Keys() const { return keys_; }
};
// MemBlindRotationEvaluationKeySet (keys.go:32)
struct MemBlindRotationEvaluationKeySet {
    RGSWKeySet rgsw;
    GaloisKeySet galois;
};
// batch entry b of ctIn through rlwe.Evaluator.Automorphism with key sel[b] of the set; sel[b] == -1 passes the entry through
inline void AutomorphismSelect(const hering::Evaluator &ev, const Ciphertext &ctIn, const GaloisKeySet &keys, const std::vector<int32_t> &sel,
                               Ciphertext &opOut) {
    check(he_automorphism_ct_select(ev.h(), ctIn.Value.at(0).h(), ctIn.Value.at(1).h(), keys.h(), sel.data(), (int)sel.size(),
                                    opOut.Value.at(0).h(), opOut.Value.at(1).h()));
}
// GenEvaluationKeyNew (keys.go:46-108; hering_rgsw_encryptor.h): RGSW(X^s[i]) for every coefficient of skLWE (a key of the ring
// paramsLWE; limb 0 of its Q part is read) and the Galois keys of 5^1 .. 5^10 and 2N - 5, under skRLWE.  prng serves the RGSW
// ciphertexts and prngKeyGen the Galois keys; given one source for both, the RGSW ciphertexts draw first.
inline MemBlindRotationEvaluationKeySet GenEvaluationKeyNew(const rgsw::Evaluator &paramsRLWE, const rlwe::SecretKey &skRLWE, const Ring &paramsLWE,
                                                            const rlwe::SecretKey &skLWE, const sampling::PRNG &prng, const sampling::PRNG &prngKeyGen,
                                                            const rlwe::EvaluationKeyParameters &evkParams = {}, DiscreteGaussian Xe = {}) {
    constexpr int windowSize = 10;  // keys.go:14
    rgsw::Encryptor enc(paramsRLWE, prng, skRLWE, Xe);
    rlwe::KeyGenerator kgen(paramsRLWE, prngKeyGen, Ternary{}, Xe);
    const int n = paramsLWE.N();
    std::vector<rgsw::Ciphertext> brk;
    std::vector<he_handle> k0, k1, g;
    for (int i = 0; i < n; i++) {
        brk.push_back(rgsw::NewCiphertext(kgen, evkParams));
        k0.push_back(brk.back().Value[0].h());
        k1.push_back(brk.back().Value[1].h());
    }
    const uint64_t twoN = (uint64_t)2 * paramsRLWE.RingQ().N();
    std::vector<uint64_t> galEls;
    std::vector<EvaluationKey> gks;
    uint64_t pw = 1;
    for (int i = 0; i <= windowSize; i++) {
        pw = pw * 5 % twoN;
        galEls.push_back(i < windowSize ? pw : twoN - 5);
        gks.push_back(kgen.NewEvaluationKey(evkParams));
        g.push_back(gks.back().h());
    }
    check(he_blindrot_gen_evaluation_key(enc.h(), kgen.h(), paramsLWE.h(), skLWE.Value.Q.h(), n, k0.data(), k1.data(), g.data()));
    return MemBlindRotationEvaluationKeySet{RGSWKeySet(paramsRLWE, brk), GaloisKeySet(paramsRLWE, galEls, gks)};
}
// blindrot.Evaluator (evaluator.go:16), BlindRotateCore only
class Evaluator {
    rgsw::Evaluator ev_;

public:
    explicit Evaluator(const rgsw::Evaluator &ev) : ev_(ev) {}
    // BlindRotateCore (:135) for every batch entry of acc, in place: a holds one row of n_lwe words mod 2N per entry
    void BlindRotateCore(const std::vector<uint64_t> &a, int n_lwe, Ciphertext &acc, const MemBlindRotationEvaluationKeySet &BRK) const {
        if (n_lwe < 1 || a.size() % (size_t)n_lwe != 0) throw std::invalid_argument("BlindRotateCore: rows of n_lwe words");
        check(he_blind_rotate_core(ev_.h(), a.data(), (int)(a.size() / (size_t)n_lwe), n_lwe, acc.Value.at(0).h(), acc.Value.at(1).h(),
                                   BRK.rgsw.h(), BRK.galois.h()));
    }
};
}  // namespace blindrot

// ---- linear transformations (circuits/common/lintrans; hering_lintrans.h), NTT domain ----------------------------------------
namespace lintrans {
// BSGSIndex (lintrans.go:344): the sorted giant steps and baby steps
inline std::pair<std::vector<int>, std::vector<int>> BSGSIndex(const std::vector<int> &nonZeroDiags, int slots, int N1) {
    std::vector<int> r1(nonZeroDiags.size() + 1), r2(nonZeroDiags.size() + 1);
    int n1 = 0, n2 = 0;
    check(he_lintrans_bsgs_index(nonZeroDiags.data(), (int)nonZeroDiags.size(), slots, N1, r1.data(), &n1, r2.data(), &n2, nullptr));
    r1.resize((size_t)n1); r2.resize((size_t)n2);
    return {r1, r2};
}
// FindBestBSGSRatio (lintrans.go:321)
inline int FindBestBSGSRatio(const std::vector<int> &nonZeroDiags, int maxN, int logMaxRatio) {
    int N1 = 0;
    check(he_lintrans_find_best_bsgs_ratio(nonZeroDiags.data(), (int)nonZeroDiags.size(), maxN, logMaxRatio, &N1));
    return N1;
}
// GaloisElements (lintrans.go:297) on the evaluator's ring
inline std::vector<uint64_t> GaloisElements(const hering::Evaluator &ev, const std::vector<int> &diags, int slots, int logBSGSRatio) {
    std::vector<uint64_t> out(2 * diags.size() + 2);
    size_t n = 0;
    check(he_lintrans_galois_elements(ev.h(), diags.data(), (int)diags.size(), slots, logBSGSRatio, out.data(), out.size(), &n));
    out.resize(n);
    return out;
}
// LinearTransformation (lintrans.go:127) over encoded diagonals (NTT + Montgomery) the caller keeps as polynomials: diag[k] is the
// index of (Q[k], P[k]).  The handle keeps them alive and reads their words when the transformation is evaluated.
class LinearTransformation {
    detail::Ref r_;
    std::vector<Poly> q_, p_;

public:
    int LevelQ, LevelP, LogSlots, N1;
    LinearTransformation(const hering::Evaluator &ev, int levelQ, int levelP, int logSlots, int n1, const std::vector<int> &diag,
                         const std::vector<Poly> &Q, const std::vector<Poly> &P)
        : q_(Q), p_(P), LevelQ(levelQ), LevelP(levelP), LogSlots(logSlots), N1(n1) {
        if (diag.size() != Q.size() || diag.size() != P.size()) throw std::invalid_argument("LinearTransformation: one (Q, P) pair per diagonal");
        std::vector<he_handle> hq, hp;
        for (const Poly &x : Q) hq.push_back(x.h());
        for (const Poly &x : P) hp.push_back(x.h());
        he_handle h = 0;
        check(he_lintrans_create(ev.h(), levelQ, levelP, logSlots, n1, (int)diag.size(), diag.data(), hq.data(), hp.data(), &h));
        r_ = detail::own(h, he_lintrans_destroy);
    }
    he_handle h() const { return r_->h; }
    // giant steps per launch of the grouped kernel: 0 (the library's default), 1, 2 or 4
    void SetGroup(int G) const { check(he_lintrans_set_group(r_->h, G)); }
};
// lintrans.Evaluator (lintrans_evaluator.go:12): EvaluateMany is ONE native call
class Evaluator {
    hering::Evaluator ev_;
    blindrot::GaloisKeySet gks_;

public:
    Evaluator(const hering::Evaluator &ev, const blindrot::GaloisKeySet &gks) : ev_(ev), gks_(gks) {}
    // :27: ctIn at ctLevel; opOut[k] = linearTransformations[k] x ctIn
    void EvaluateMany(int ctLevel, const Ciphertext &ctIn, const std::vector<LinearTransformation> &linearTransformations,
                      std::vector<Ciphertext> &opOut) const {
        if (opOut.size() < linearTransformations.size()) throw std::invalid_argument("output *rlwe.Ciphertext slice is too small");
        std::vector<he_handle> lts, o0, o1;
        for (size_t k = 0; k < linearTransformations.size(); k++) {
            lts.push_back(linearTransformations[k].h());
            o0.push_back(opOut[k].Value.at(0).h());
            o1.push_back(opOut[k].Value.at(1).h());
        }
        check(he_lintrans_evaluate_many(ev_.h(), gks_.h(), ctLevel, ctIn.Value.at(0).h(), ctIn.Value.at(1).h(), (int)lts.size(), lts.data(),
                                        o0.data(), o1.data()));
    }
    // :122
    void Evaluate(int ctLevel, const Ciphertext &ctIn, const LinearTransformation &lt, Ciphertext &opOut) const {
        check(he_lintrans_evaluate(ev_.h(), gks_.h(), ctLevel, ctIn.Value.at(0).h(), ctIn.Value.at(1).h(), lt.h(), opOut.Value.at(0).h(),
                                   opOut.Value.at(1).h()));
    }
    // :128: each transformation on the result of the one before; opOut receives the last result (the caller rescales between two
    // of them where the scheme wants it: pass one transformation at a time then)
    void EvaluateSequential(int ctLevel, const Ciphertext &ctIn, const std::vector<LinearTransformation> &linearTransformations,
                            Ciphertext &opOut) const {
        if (linearTransformations.empty()) return;
        Evaluate(ctLevel, ctIn, linearTransformations[0], opOut);
        int level = std::min(ctLevel, linearTransformations[0].LevelQ);
        for (size_t k = 1; k < linearTransformations.size(); k++) {  // in place: n_lt = 1 takes the outputs on the inputs
            Evaluate(level, opOut, linearTransformations[k], opOut);
            level = std::min(level, linearTransformations[k].LevelQ);
        }
    }
};
}  // namespace lintrans

// ---- polynomial evaluation (circuits/common/polynomial; hering_polyeval.h), NTT domain ---------------------------------------
namespace polyeval {
// bignum.OptimalSplit (utils/bignum/polynomial.go:14)
inline int OptimalSplit(int logDegree) {
    int s = 0;
    check(he_polyeval_optimal_split(logDegree, &s));
    return s;
}
// SplitDegree (power_basis.go:31)
inline std::pair<int, int> SplitDegree(int n) {
    int a = 0, b = 0;
    check(he_polyeval_split_degree(n, &a, &b));
    return {a, b};
}
// ceil(log2 degree); throws the reference's error where `level` is below it (polynomial_evaluator.go:62-65)
inline int Depth(int degree, int level) {
    int d = 0;
    check(he_polyeval_depth(degree, level, &d));
    return d;
}
// one power a basis holds: X^n at a level, as a ciphertext of degree 1 or 2
struct PowerInfo { int n, level, degree; };
struct LeafInfo { int degree, level, new_degree, ct_degree; uint32_t present; };
struct Step { int op, dst, level, degree, a, b; };
// the library's structure of one evaluation (he_debug_polyeval_plan)
struct Plan {
    int log_split = 0, depth = 0, out_level = 0;
    std::vector<LeafInfo> leaves;
    std::vector<Step> steps;
    Plan(int degree, int basis, bool even, bool odd, bool lazy, const std::vector<PowerInfo> &powers, bool copyInput) {
        std::vector<int> flat;
        for (const PowerInfo &p : powers) { flat.push_back(p.n); flat.push_back(p.level); flat.push_back(p.degree); }
        size_t n = 0;
        check(he_polyeval_plan(degree, basis, even, odd, lazy, copyInput, (int)powers.size(), flat.data(), nullptr, 0, &n));
        std::vector<int64_t> w(n);
        check(he_polyeval_plan(degree, basis, even, odd, lazy, copyInput, (int)powers.size(), flat.data(), w.data(), n, &n));
        log_split = (int)w[0]; depth = (int)w[1]; out_level = (int)w[4];
        size_t at = 5;
        for (int64_t i = 0; i < w[2]; i++, at += 5) leaves.push_back({(int)w[at], (int)w[at + 1], (int)w[at + 2], (int)w[at + 3], (uint32_t)w[at + 4]});
        for (int64_t i = 0; i < w[3]; i++, at += 6) steps.push_back({(int)w[at], (int)w[at + 1], (int)w[at + 2], (int)w[at + 3], (int)w[at + 4], (int)w[at + 5]});
    }
};
// BGV planning of the scalar words (circuits/bgv/polynomial): residues mod t, centred, the op0.Scale != opOut.Scale ratio of
// MulThenAdd (schemes/bgv/evaluator.go:1108-1140) and the constant of Add (:144-172) times T^-1 mod Q_level.  tInvModQ[l][i] =
// (T^-1 mod q_0 ... q_l) mod q_i, which the caller computes with its big integers.
struct BGVWords {
    uint64_t t;
    std::vector<uint64_t> Q;
    static uint64_t mulmod(uint64_t a, uint64_t b, uint64_t m) { return (uint64_t)((unsigned __int128)a * b % m); }
    static uint64_t powmod(uint64_t a, uint64_t e, uint64_t m) {
        uint64_t r = 1 % m;
        for (a %= m; e; e >>= 1, a = mulmod(a, a, m))
            if (e & 1) r = mulmod(r, a, m);
        return r;
    }
    // the residue of the centred representative of v mod t, modulo q
    uint64_t centred(uint64_t v, uint64_t q) const {
        v %= t;
        return v > (t >> 1) ? (q - (t - v) % q) % q : v % q;
    }
    // MulThenAdd(X, c, out): the words of c at (X.Scale, out.Scale)
    std::vector<uint64_t> term(int level, uint64_t c, uint64_t xScale, uint64_t outScale) const {
        uint64_t v = c % t;
        if (xScale != outScale) v = mulmod(v, mulmod(powmod(xScale, t - 2, t), outScale, t), t);
        std::vector<uint64_t> w;
        for (int i = 0; i <= level; i++) w.push_back(centred(v, Q[(size_t)i]));
        return w;
    }
    // Add(out, c): the words of c at out.Scale
    std::vector<uint64_t> constant(int level, uint64_t c, uint64_t outScale, const std::vector<uint64_t> &tInvModQ) const {
        const uint64_t v = mulmod(c % t, outScale % t, t);
        std::vector<uint64_t> w;
        for (int i = 0; i <= level; i++) w.push_back(mulmod(centred(v, Q[(size_t)i]), tInvModQ[(size_t)i], Q[(size_t)i]));
        return w;
    }
};
// the caller's numbers for the Chebyshev steps of a plan, in its order (hering_polyeval.h): kind 0 = Add(x, -1), 1 / 2 = Sub with the
// second / first operand times the integer ratio first, 3 = Sub as it is; `words` residues per entry in s0 and s1
struct ChebyshevWords {
    std::vector<int> kind;
    std::vector<uint64_t> s0, s1;
    int words = 0;
};
// polynomial.PowerBasis (power_basis.go:17) on the device: NewPowerBasis copies the ciphertext into X^1
class PowerBasis {
    detail::Ref r_;

public:
    PowerBasis(const hering::Evaluator &ev, int basis, int level, const Ciphertext &ct) {
        he_handle h = 0;
        check(he_polyeval_basis_create(ev.h(), basis, level, ct.Value.at(0).h(), ct.Value.at(1).h(), &h));
        r_ = detail::own(h, he_polyeval_basis_destroy);
    }
    he_handle h() const { return r_->h; }
    // the powers the basis holds
    std::vector<PowerInfo> Powers() const {
        size_t n = 0;
        check(he_polyeval_basis_powers(r_->h, nullptr, 0, &n));
        std::vector<int> w(3 * n + 3);
        check(he_polyeval_basis_powers(r_->h, w.data(), n, &n));
        std::vector<PowerInfo> out;
        for (size_t i = 0; i < n; i++) out.push_back({w[3 * i], w[3 * i + 1], w[3 * i + 2]});
        return out;
    }
    // GenPower (power_basis.go:76): scheme 0 CKKS, 1 BGV with plaintext modulus t; rlk may be null where nothing is relinearized
    void GenPower(int scheme, uint64_t t, const EvaluationKey *rlk, int n, bool lazy, const ChebyshevWords &cw = {}) const {
        check(he_polyeval_gen_power(r_->h, scheme, t, rlk ? rlk->h() : 0, n, lazy, (int)cw.kind.size(), cw.kind.data(), cw.s0.data(), cw.s1.data(), cw.words));
    }
};
// A polynomial planned for one basis, its scalar words uploaded once (he_polyeval_poly_create): s0 / s1 hold, per baby step in
// the library's order and per coefficient k = 0 .. degree, 1 + level(X^1) residues (BGV: s1 = s0; CKKS: the planned pairs)
class Polynomial {
    detail::Ref r_;

public:
    Polynomial(const Ring &ring, int degree, int basis, bool even, bool odd, bool lazy, const std::vector<PowerInfo> &powers,
               const std::vector<int> &leafDegree, const std::vector<int> &leafLevel, const std::vector<uint64_t> &s0, const std::vector<uint64_t> &s1) {
        if (leafDegree.size() != leafLevel.size()) throw std::invalid_argument("Polynomial: one level per baby step");
        std::vector<int> flat;
        for (const PowerInfo &p : powers) { flat.push_back(p.n); flat.push_back(p.level); flat.push_back(p.degree); }
        he_handle h = 0;
        check(he_polyeval_poly_create(ring.h(), degree, basis, even, odd, lazy, (int)powers.size(), flat.data(), (int)leafDegree.size(),
                                      leafDegree.data(), leafLevel.data(), s0.data(), s1.data(), &h));
        r_ = detail::own(h, he_polyeval_poly_destroy);
    }
    he_handle h() const { return r_->h; }
    // baby steps per launch of the leaf-group kernel: 0 (the library's default), 1, 2 or 4
    void SetGroup(int G) const { check(he_polyeval_poly_set_group(r_->h, G)); }
    // EvaluatePolynomialVectorFromPowerBasis (polynomial_evaluator.go:254) for the baby steps [first, first + out.size()): X[k - 1]
    // = the power X^k (an empty ciphertext where the basis lacks it), out[g] = the result of baby step first + g
    void EvaluatePolynomialFromPowerBasis(int first, const std::vector<Ciphertext> &X, std::vector<Ciphertext> &out) const {
        std::vector<he_handle> x(3 * X.size() + 1, 0), o(3 * out.size() + 1, 0);
        for (size_t k = 0; k < X.size(); k++)
            for (size_t c = 0; c < X[k].Value.size() && c < 3; c++) x[3 * k + c] = X[k].Value[c].h();
        for (size_t g = 0; g < out.size(); g++)
            for (size_t c = 0; c < out[g].Value.size() && c < 3; c++) o[3 * g + c] = out[g].Value[c].h();
        check(he_polyeval_leaves(r_->h, first, (int)out.size(), (int)X.size(), x.data(), o.data()));
    }
    // Evaluator.Evaluate (polynomial_evaluator.go:33) as ONE native call: ct at `level` is left untouched, opOut receives the result
    void Evaluate(const hering::Evaluator &ev, int scheme, uint64_t t, const EvaluationKey *rlk, int level, const Ciphertext &ct,
                  const ChebyshevWords &cw, Ciphertext &opOut) const {
        check(he_polyeval_evaluate(ev.h(), r_->h, scheme, t, rlk ? rlk->h() : 0, level, ct.Value.at(0).h(), ct.Value.at(1).h(), (int)cw.kind.size(),
                                   cw.kind.data(), cw.s0.data(), cw.s1.data(), cw.words, opOut.Value.at(0).h(), opOut.Value.at(1).h()));
    }
    // Evaluator.EvaluateFromPowerBasis (:47) as ONE native call on the basis the polynomial was planned for
    void EvaluateFromPowerBasis(const PowerBasis &pb, int scheme, uint64_t t, const EvaluationKey *rlk, const ChebyshevWords &cw, Ciphertext &opOut) const {
        check(he_polyeval_evaluate_from_power_basis(pb.h(), r_->h, scheme, t, rlk ? rlk->h() : 0, (int)cw.kind.size(), cw.kind.data(), cw.s0.data(),
                                                    cw.s1.data(), cw.words, opOut.Value.at(0).h(), opOut.Value.at(1).h()));
    }
};
}  // namespace polyeval

// ---- ckks.Evaluator (schemes/ckks/evaluator.go; hering_ckks_evaluator.h), NTT domain -------------------------------------------
// The linear forms over a whole ciphertext and MulRelinThenAdd, one launch each.  The caller plans levels, scales and the residues
// of scalars, ratios and scale-ups (as lattigo_amd.ckks.Evaluator does); every word list holds one residue per limb 0 .. level.
namespace ckks {
class Evaluator {
    Ring ringQ_;
    const hering::Evaluator *ev_;

    static std::vector<he_handle> handles(const std::vector<Poly> &v) {
        std::vector<he_handle> h;
        for (const Poly &p : v) h.push_back(p.h());
        return h;
    }
    static const uint64_t *words(const std::vector<uint64_t> *w) { return w ? w->data() : nullptr; }

public:
    // ringQ: Parameters.RingQ(); ev: the rlwe evaluator of the parameters (MulRelinThenAdd only; may be null otherwise)
    Evaluator(const Ring &ringQ, const hering::Evaluator *ev = nullptr) : ringQ_(ringQ), ev_(ev) {}
    // evaluateInPlace (:221-408) with Ring.Add / Ring.Sub; scaled = 1 / 2: op0 / op1 is first multiplied by the integer `ratio`
    void AddSub(int level, bool sub, const Ciphertext &op0, const Ciphertext &op1, int scaled, const std::vector<uint64_t> *ratio,
                Ciphertext &opOut) const {
        const auto a = handles(op0.Value), b = handles(op1.Value), o = handles(opOut.Value);
        check(he_ckks_add(ringQ_.h(), level, sub ? 1 : 0, (int)a.size(), a.data(), (int)b.size(), b.data(), scaled, words(ratio), (int)o.size(),
                          o.data()));
    }
    // evaluateWithScalar (:410-424): op = HE_CKKS_SCALAR_*; (s0, s1): the scalar on the two halves of a limb; pre: the scale-up of
    // opOut before MUL_THEN_ADD (:959-964)
    void Scalar(int level, int op, const Ciphertext &op0, const std::vector<uint64_t> &s0, const std::vector<uint64_t> &s1,
                const std::vector<uint64_t> *pre, Ciphertext &opOut) const {
        const auto a = handles(op0.Value), o = handles(opOut.Value);
        if (a.size() != o.size()) throw std::invalid_argument("ckks::Evaluator::Scalar: op0 and opOut differ in degree");
        check(he_ckks_scalar(ringQ_.h(), level, op, (int)a.size(), a.data(), s0.data(), s1.data(), words(pre), o.data()));
    }
    // the plaintext branches of mulRelin (:842-869) and mulRelinThenAdd (:1158-1170)
    void MulPlaintext(int level, const Ciphertext &ct, const Poly &pt, bool thenAdd, const std::vector<uint64_t> *pre, Ciphertext &opOut) const {
        const auto a = handles(ct.Value), o = handles(opOut.Value);
        if (a.size() != o.size()) throw std::invalid_argument("ckks::Evaluator::MulPlaintext: ct and opOut differ in degree");
        check(he_ckks_mul_pt(ringQ_.h(), level, (int)a.size(), a.data(), pt.h(), thenAdd ? 1 : 0, words(pre), o.data()));
    }
    // the ciphertext x ciphertext branch of mulRelinThenAdd (:1104-1155); rlk null: MulThenAdd onto three components
    void MulRelinThenAdd(int level, const Ciphertext &op0, const Ciphertext &op1, const EvaluationKey *rlk, const std::vector<uint64_t> *pre,
                         Ciphertext &opOut) const {
        if (!ev_) throw std::invalid_argument("ckks::Evaluator::MulRelinThenAdd: no rlwe evaluator");
        check(he_ckks_mul_relin_then_add(ev_->h(), level, op0.Value.at(0).h(), op0.Value.at(1).h(), op1.Value.at(0).h(), op1.Value.at(1).h(),
                                         rlk ? rlk->h() : 0, words(pre), opOut.Value.at(0).h(), opOut.Value.at(1).h(),
                                         rlk ? 0 : opOut.Value.at(2).h()));
    }
};
}  // namespace ckks

// One process per GPU: the RCCL communicator of a context, driven by the library on the context's stream (key replication over xGMI;
// the all-reduce of a key switch split by digit).  Rank 0 draws the id and hands it to the others over any control plane.
class Communicator {
    detail::Ref r_;

public:
    static bool Available() {
        int yes = 0;
        check(he_rccl_available(&yes));
        return yes != 0;
    }
    static std::array<uint8_t, HE_RCCL_ID_BYTES> UniqueId() {
        std::array<uint8_t, HE_RCCL_ID_BYTES> id{};
        check(he_rccl_unique_id(id.data()));
        return id;
    }
    Communicator(const Context &ctx, const std::array<uint8_t, HE_RCCL_ID_BYTES> &id, int rank, int world) {  // collective
        he_handle h = 0;
        check(he_rccl_comm_create(ctx.h(), id.data(), rank, world, &h));
        r_ = detail::own(h, he_rccl_comm_destroy);
    }
    int Ranks() const {  // the ranks RCCL itself reaches (an all-reduce of ones)
        int n = 0;
        check(he_rccl_comm_ranks(r_->h, &n));
        return n;
    }
    void Broadcast(const EvaluationKey &evk, int root) const { check(he_evk_broadcast(r_->h, evk.h(), root)); }
    void AllReduceSum(Poly &p) const { check(he_poly_all_reduce_sum(r_->h, p.h())); }
};

}  // namespace hering
#endif  // HERING_HPP
