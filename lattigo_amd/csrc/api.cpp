// api.cpp -- the C ABI of libhering (include/hering.h): handle registry, device-resident
// ring / poly / key objects and the host-side orchestration of the kernels in
// kernels.hip.  Mirrors the reference's ring.Ring / ring.BasisExtender / ring.Decomposer /
// rlwe.Evaluator call structure (file:line cited per function) with every loop over
// coefficients replaced by a launch covering all (limb x batch entry) pairs.
//
// There is NO CPU fallback: every arithmetic entry point enqueues gfx950 kernels; if the
// HIP runtime or device is missing the call fails with HE_EDEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <tuple>
#include <mutex>
#include <numeric>
#include <shared_mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <cstdlib>
#include <vector>
#include <dlfcn.h>
#include <pthread.h>
#include <sched.h>
#include <climits>
#include <linux/futex.h>
#include <sys/random.h>
#include <sys/syscall.h>
#include <unistd.h>

#include "../../include/hering.h"
#include "../../include/hering_debug.h"
#include "../../include/hering_ringswitch.h"
#include "../../include/hering_bridge.h"
#include "../../include/hering_bfv.h"
#include "../../include/hering_ckks_encoder.h"
#include "../../include/hering_bgv_encoder.h"
#include "../../include/hering_sampler.h"
#include "../../include/hering_encryptor.h"
#include "../../include/hering_keygen.h"
#include "../../include/hering_rgsw_encryptor.h"
#include "../../include/hering_multiparty.h"
#include "../../include/hering_ringpack.h"
#include "../../include/hering_rgsw.h"
#include "../../include/hering_blindrot.h"
#include "../../include/hering_lintrans.h"
#include "../../include/hering_polyeval.h"
#include "../../include/hering_ckks_evaluator.h"
#include "host_math.h"
#include "kernels.h"
#include "ks_route.h"
#include "blindrot_plan.h"
#include "lintrans_plan.h"
#include "polyeval_plan.h"

using namespace he;

namespace {

thread_local std::string g_err;
int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) return fail(HE_EDEVICE, "%s: %s", #expr, hipGetErrorString(_e));    \
    } while (0)
#define TRY(expr)              \
    do {                       \
        int _r = (expr);       \
        if (_r != HE_OK) return _r; \
    } while (0)

enum ObjType { T_CTX = 1, T_RING, T_POLY, T_INDEX, T_BE, T_EVAL, T_EVK, T_DECOMP, T_GRAPH, T_COMM, T_RGSW_SET, T_GALOIS_SET, T_BFV, T_CKKS_ENC, T_BGV_ENC, T_PRNG, T_ENCRYPTOR, T_DECRYPTOR, T_KEYGEN, T_LINTRANS, T_POLYEVAL, T_POLYBASIS };

struct Obj {
    ObjType type;
    explicit Obj(ObjType t) : type(t) {}
    virtual ~Obj() {}
};

// Submission queue of a context (he_ctx_set_coalescing / he_evaluator_set_coalescing): concurrent single-ciphertext calls of one
// operation are gathered into ONE batched launch over an entry table of the callers' own polynomials (View::tab).  The reference's
// unit of parallelism is a goroutine per ciphertext on CPU cores (b.RunParallel, schemes/ckks/ckks_benchmarks_test.go:116-207, over
// evaluators that share their tables, core/rlwe/evaluator.go:200-227; the bootstrapping benchmark runs whole circuits that way,
// circuits/ckks/bootstrapping/evaluator_benchmarks_test.go:14-42); a GPU wants those callers in one grid.  Flat combining:
// a caller files its request; whoever finds no leader becomes the leader, gathers for at most `window_us` (no limit while two
// earlier batches are still in flight on the device -- waiting is free then), launches every pending request of the oldest
// request's key as one batch, marks them done and hands the role over.  A call returns once its batch is ENQUEUED on the
// context's stream (the library's usual contract: results are visible after he_ctx_sync / a download).
//
// Round 5: the queue belongs to the CONTEXT and a request is generic -- (operation, the object it addresses, its scalar
// arguments) is the key, the operands are a list of device views, and the launches are a closure over everything in the key that
// is handed the operands as views (one request: its own; a batch: entry 0's base pointers + entry tables).  Every entry point of
// the one-ciphertext interface files such a request (the ring-level methods, Rescale, the seven rlwe.EvaluatorProvider methods,
// the lintrans inner loop), not only the four key switches of round 4.
enum CoOp {
    CO_MUL_RELIN = 0, CO_GADGET_PRODUCT, CO_RELINEARIZE, CO_AUTOMORPHISM,
    CO_NTT, CO_EW, CO_EW_DOUBLE, CO_SHIFT, CO_RESCALE, CO_GATHER, CO_AUTO_COEFF, CO_MODUP, CO_MODDOWN_BE,
    CO_DECOMPOSE_SPLIT, CO_DECOMPOSE_NTT, CO_GP_LAZY, CO_GP_HOISTED_LAZY, CO_GP_HOISTED, CO_MODDOWN, CO_EVAL_MODDOWN,
    CO_AUTO_HOISTED, CO_AUTO_HOISTED_LAZY, CO_CENTERED_LIFT, CO_DECOMP_FILL, CO_LINTRANS, CO_MUL, CO_COPY, CO_ZERO, CO_GIANT_STEP,
    CO_RING_SWITCH, CO_APPLY_EVK, CO_RING_PACK, CO_RINGPACK_CT, CO_RGSW, CO_AUTO_SELECT, CO_BLINDROT,
    CO_CI_BRIDGE, CO_CI_BRIDGE_CT, CO_BFV_MUL, CO_BFV_QUANTIZE, CO_LINTRANS_EVAL, CO_POLY_LEAVES, CO_CT_LIN, CO_TENSOR_ADD
};
// kinds of CO_RING_PACK (par[0]): the entries of include/hering_ringpack.h that address a ring
enum { RP_XPOW2 = 0, RP_SPLIT, RP_MERGE, RP_EXPAND, RP_PACK_PRE, RP_PACK_POST };
struct CoReq {
    // ---- key: requests are batched together only when all of this matches
    int op = 0;
    const void *obj = nullptr;      // the ring / basis extender / evaluator the call addresses
    const void *key = nullptr;      // evaluation key (or index table) identity
    int64_t par[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // the call's scalar arguments; par[7] = aliasing pattern of the operands
    std::vector<uint64_t> blob;     // scalar arguments of variable size (per-limb scalars, ...), compared by value
    // ---- operands: device views of this request's own polynomials (null pointer: operand absent)
    std::vector<View> ops;
    int nb = 1;  // batch entries of this request's handles (entry i of operand s: ops[s].p + i * ops[s].bstride)
    std::vector<std::shared_ptr<Obj>> keep;  // what the launches address stays alive until they are enqueued
    // the launches over B entries, v[s] = operand s (this request's views, or entry 0's pointer + an entry table).  It must
    // capture nothing that is not covered by the key: a batch runs the closure of its FIRST request for everyone.
    std::function<int(const View *v, int B)> run;
    // optional: may this shape be addressed through entry tables (false: the batch is served one by one)?
    std::function<int(bool *ok)> tables_ok;
    // a batch of this request is served one by one: its launches take no entry tables
    void one_by_one() { tables_ok = [](bool *ok) -> int { *ok = false; return HE_OK; }; }
    // ---- queue state
    std::chrono::steady_clock::time_point arrived;
    uint64_t caller = 0;  // the submitting thread (several requests of one call share it)
    uint64_t seq = 0;     // how many queued calls that thread had made before this one
    uint64_t ticket = 0;  // deferred submission: filing order over all threads of the context (he_ctx_sync waits by ticket)
    // done: status and message are final (the LAST thing a leader writes: the submitter may return, and the request die, at once);
    // lead: the leaving leader handed the role to this (still waiting) request.  Both are read without the queue's lock by the
    // sleeping submitter, which waits on the queue's generation word (Coalescer::gen).
    std::atomic<bool> done{false}, lead{false};
    int rc = 0;
    std::string err;
    bool same_key(const CoReq &o) const {
        return op == o.op && obj == o.obj && key == o.key && memcmp(par, o.par, sizeof par) == 0 && ops.size() == o.ops.size() &&
               blob == o.blob;
    }
    // par[7]: which operands are the same polynomial (bit i * n + j for i < j): the launches decide in-place forms on entry 0's
    // pointers, so every entry of a batch must alias the same way.  The first 11 operands give 55 bits; a request with more
    // (CO_LINTRANS: 4 + 6 n) adds the rest of its pattern to the blob -- per operand, the first operand with the same storage --
    // so that requests of different patterns never share a batch, whatever the operation does with them.
    void set_alias_pattern() {
        uint64_t m = 0;
        int bit = 0;
        const size_t n = ops.size() < 11 ? ops.size() : 11;
        for (size_t i = 0; i < n; i++)
            for (size_t j = i + 1; j < n; j++, bit++)
                if (ops[i].p && ops[i].p == ops[j].p) m |= 1ull << bit;
        par[7] = (int64_t)m;
        if (ops.size() > 11) {
            std::unordered_map<const uint64_t *, uint64_t> first;
            for (size_t i = 0; i < ops.size(); i++)
                blob.push_back(ops[i].p ? first.emplace(ops[i].p, (uint64_t)i).first->second : UINT64_MAX);
        }
    }
};
struct Coalescer {
    std::mutex mu;
    std::condition_variable cv_leader;  // the gathering leader waits here for arrivals while the device is busy
    // Submitters sleep on this word (futex): a finished batch or a hand-over of the leader's role bumps it and wakes them ALL with
    // one system call; each looks at its own request's flags and goes back to sleep if it is not concerned.  (Round 4 had one
    // condition variable per request: a batch of 64 cost its leader 64 wake-up calls under the queue's lock, and every woken
    // caller queued for that lock first -- 0.3 ms per batch once the batches themselves took less.)
    std::atomic<uint32_t> gen{0};
    std::deque<CoReq *> pending;
    bool leader = false;
    int recent[4] = {0, 0, 0, 0};     // sizes of the last batches: callers that wait for their results come back together
    // read without the lock by every single-ciphertext call that asks "is the queue on?": atomic.  0 / 1 = off.
    std::atomic<int> max_batch{0};
    int window_us = 0;
    // entry tables: kTabSlots slots of [rows][B] word offsets in one allocation.  A batch whose offsets equal those of a slot
    // (callers that loop over the same polynomials: the same table every round) reuses it without a fill launch; otherwise the
    // least recently used slot is refilled -- in stream order, after the launches that read its old contents.
    static constexpr int kTabSlots = 16;
    size_t *d_tab = nullptr;
    size_t tab_words = 0;     // capacity of ONE slot: a batch whose table does not fit is served one by one
    struct TabSlot { std::vector<size_t> vals; uint64_t used = 0; };
    TabSlot tab_slot[kTabSlots];
    uint64_t tab_clock = 0, tab_hits = 0, tab_fills = 0;  // (under the context's lock, like the launches)
    std::deque<hipEvent_t> inflight;  // one event per launched batch, oldest first
    std::vector<hipEvent_t> free_events;
    uint64_t n_calls = 0, n_launches = 0, n_max = 0, n_fallback = 0;  // he_ctx_coalescing_stats
    // > 0 while recent traffic showed callers overlapping (a batch of more than one request, or requests left waiting when a
    // batch was taken): a lone caller -- no one to wait for -- is launched without the gathering window
    int crowd = 0;
    // the threads that filed a request lately (id, time of their last request): the gathering rule waits for them
    std::vector<std::pair<uint64_t, std::chrono::steady_clock::time_point>> seen;
    // diagnosis (he_debug_queue_counters): why gathering ended -- [0] everyone here, [1] timeout, [2] full -- and where the
    // leaders' time went: [3] microseconds gathering, [4] microseconds launching, [5] sum of callers present, [6] sum of callers expected
    // deferred mode: [8] us the dispatcher paused because it was four batches ahead of the device, [9] us it waited for callers
    // while the device had two or more batches queued (free), [10] us it waited for callers with the device running dry, [11] batches
    // [12] (HERING_QUEUE_TIMING=1 only) device microseconds between the first and the last launch of the batches, as the stream ran them
    std::atomic<uint64_t> dbg[16] = {};  // (the dispatcher adds to them outside the queue's lock)
    uint64_t op_launches[32] = {0}, op_calls[32] = {0};  // per operation (CoOp): batches launched, requests served (he_debug_queue_op_stats)
    std::deque<hipEvent_t> inflight_begin;  // HERING_QUEUE_TIMING=1: the event recorded before each batch of `inflight`
    // ---- deferred submission (he_ctx_set_deferred): a call files its request and RETURNS; a dispatcher thread of the context
    // gathers and launches.  depth: requests one thread may have pending before its next call waits (0: off -- calls wait for
    // their launch as above).  A thread's requests are launched in the order it made them; only the first pending call of each
    // thread is a candidate for a batch.
    std::atomic<int> depth{0};
    std::thread dispatcher;
    std::atomic<bool> stop{false};
    std::atomic<uint64_t> next_ticket{1};
    std::atomic<uint64_t> launching_min{UINT64_MAX};  // smallest ticket of the batch being launched right now
    // one record per calling thread (never freed while the context lives: the thread keeps the pointer): its requests in the
    // order it made them -- under ITS OWN lock, so that filing a request contends with nobody but the dispatcher's glance at this
    // queue (64 callers filing through the queue's one mutex spent two thirds of their CPU time in futex calls) -- how many of
    // them are not launched yet, whether it sleeps until that count falls to half of `depth`, and when it last filed
    struct Caller {
        std::atomic<uint64_t> id{0};  // the thread it belongs to; 0: free (its thread ended with nothing pending), may be claimed
        std::mutex mu;
        std::deque<CoReq *> q;
        std::atomic<int> pending{0};
        std::atomic<bool> wait_low{false};
        std::atomic<int64_t> last_us{0};
    };
    static constexpr int kMaxCallers = 2048;          // threads beyond that go the blocking way
    std::atomic<Caller *> callers[kMaxCallers];
    std::atomic<int> n_callers{0};
    const uint64_t uid;                               // identity for the threads' caches of their record (an address can be reused)
    std::atomic<int> n_deferred{0};                   // requests in the callers' queues
    std::atomic<uint32_t> work{0};                    // bumped by every filed call: the dispatcher sleeps on it
    std::atomic<bool> disp_idle{false};
    std::shared_mutex life;                           // filing holds it shared; switching deferred mode off takes it exclusively
    std::atomic<int> sleepers{0};                     // threads asleep on `gen`
    std::atomic<int> flushers{0};                     // threads that wait for launches (a flush): woken after every batch
    int def_rc = 0;                                   // first failure of a deferred launch: reported by the next he_ctx_sync
    std::string def_err;
    static uint64_t new_uid() { static std::atomic<uint64_t> n{1}; return n.fetch_add(1, std::memory_order_relaxed); }
    // the queues alive in this process, by uid: a thread that ends gives its records back (co_thread_exit)
    static std::mutex &live_mu() { static std::mutex m; return m; }
    static std::unordered_map<uint64_t, Coalescer *> &live() { static std::unordered_map<uint64_t, Coalescer *> m; return m; }
    Coalescer() : uid(new_uid()) {
        for (auto &c : callers) c.store(nullptr, std::memory_order_relaxed);
        std::lock_guard<std::mutex> lk(live_mu());
        live()[uid] = this;
    }
    ~Coalescer() {
        { std::lock_guard<std::mutex> lk(live_mu()); live().erase(uid); }
        for (int i = 0; i < n_callers.load(); i++) delete callers[i].load();
    }
};
thread_local bool g_dispatcher_thread = false;  // the dispatcher's own launches do not wait for the queue


struct Ctx : Obj {
    int dev = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // stream-ordered scratch arena (temporaries of one API call)
    uint64_t *arena = nullptr;
    size_t arena_words = 0, arena_used = 0;
    std::mutex mu;
    const std::unique_ptr<Coalescer> co{new Coalescer()};  // always there (off until he_ctx_set_coalescing): no pointer to race on
    // he_ctx_sync from many threads: one drains the stream, the others wait for a drain that covers their ticket
    std::mutex sync_mu;
    std::condition_variable sync_cv;
    uint64_t sync_tickets = 0, sync_covered = 0;
    bool syncing = false;
    int sync_waiters = 0;
    // Algorithmic HBM bytes of the primitives called on this context, by the per-primitive formulas of SURVEY.md section 8(d)
    // (ideal single pass: every operand read once, every result written once; twiddles / constants / index tables excluded):
    // [0] with an evaluation key charged to every batch entry, [1] with one key read serving the whole batch.  bench.py sums
    // them over a workload's operation trace (he_alg_bytes, hering_debug.h); accounted where a call takes the context lock.
    double alg_bytes[2] = {0.0, 0.0};
    // Modular-multiply work of the primitives called on this context, in closed form per primitive (NTT
    // (N/2) logN + N per limb, basis extension L_src x L_dst x N, key inner product 2 beta (L + alpha) N, tensor 6 L N, ...), by
    // the arithmetic class of the limb it runs on: [0] multiply-equivalents on integer-class limbs (64-bit Montgomery products),
    // [1] on limbs below 2^47 (exact double-precision products), [2] / [3] how many of those are NTT butterflies (a product plus
    // an add, a subtract and the range handling) -- he_alg_valu (hering_debug.h): bench.py's `roofline.valu` for every workload
    double alg_valu[4] = {0.0, 0.0, 0.0, 0.0};
    void acct(double per_entry_limbs, double shared_limbs, int batch, int N) {
        alg_bytes[0] += (per_entry_limbs + shared_limbs) * batch * (double)N * 8.0;
        alg_bytes[1] += (per_entry_limbs * batch + shared_limbs) * (double)N * 8.0;
    }
    // size-keyed cache of polynomial buffers: the drivers above the ABI allocate and drop temporaries per call, and
    // hipMalloc/hipFree synchronise the device.  Reuse is stream-ordered (one stream per context), so a buffer can be
    // handed out again without waiting for the kernels that last touched it.
    std::multimap<size_t, void *> pool;
    std::mutex pool_mu;  // own lock: the pool is used while an API call already holds `mu`
    // he_graph_begin .. he_graph_end: the stream is capturing.  Buffers released meanwhile are parked here instead of going back
    // to the pool -- the captured launches address them, so they belong to the graph until it is destroyed.
    bool capturing = false;
    std::vector<std::pair<size_t, void *>> capture_hold;
    // captured launches address the scratch arena too: while a graph of this context is alive, an arena that has to grow is
    // retired (kept until the last graph is destroyed) instead of freed
    int live_graphs = 0;
    std::vector<uint64_t *> retired_arenas;
    void graph_released() {
        std::lock_guard<std::mutex> lk(mu);
        if (--live_graphs > 0) return;
        hipStreamSynchronize(stream);
        for (uint64_t *a : retired_arenas) hipFree(a);
        retired_arenas.clear();
    }
    size_t pool_bytes = 0;
    std::atomic<uint64_t> pool_misses{0};  // allocations the cache could not serve (he_debug_queue_counters)
    // bound of the cache: half of the device's memory (set by he_ctx_create; 288 GB of HBM3E per MI355X).  A release beyond it has
    // to drain the stream before hipFree -- with K callers' temporaries in flight that is tens of milliseconds per call
    size_t kPoolCap = (size_t)48 << 30;
    hipError_t pool_take(size_t bytes, void **out) {
        {
            std::lock_guard<std::mutex> lk(pool_mu);
            auto it = pool.find(bytes);
            if (it != pool.end()) {
                *out = it->second;
                pool.erase(it);
                pool_bytes -= bytes;
                return hipSuccess;
            }
        }
        pool_misses.fetch_add(1, std::memory_order_relaxed);
        hipError_t e = hipMalloc(out, bytes);
        if (e != hipSuccess) {  // give the cache back to the driver and retry once
            (void)hipGetLastError();
            pool_release_all();
            e = hipMalloc(out, bytes);
        }
        return e;
    }
    void pool_give(size_t bytes, void *p) {
        {
            std::lock_guard<std::mutex> lk(pool_mu);
            if (capturing) { capture_hold.emplace_back(bytes, p); return; }
            if (pool_bytes + bytes <= kPoolCap) {
                pool.emplace(bytes, p);
                pool_bytes += bytes;
                return;
            }
        }
        hipStreamSynchronize(stream);
        hipFree(p);
    }
    void pool_release_all() {
        std::lock_guard<std::mutex> lk(pool_mu);
        if (stream) hipStreamSynchronize(stream);
        for (auto &kv : pool) hipFree(kv.second);
        pool.clear();
        pool_bytes = 0;
    }
    Ctx() : Obj(T_CTX) {}
    ~Ctx() override {
        if (co->dispatcher.joinable()) {  // (he_ctx_destroy stops it; this is the context dying with its last object)
            co->stop = true;
            co->work.fetch_add(1, std::memory_order_seq_cst);
            syscall(SYS_futex, reinterpret_cast<uint32_t *>(&co->work), FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
            if (co->dispatcher.get_id() == std::this_thread::get_id()) co->dispatcher.detach();
            else co->dispatcher.join();
        }
        hipSetDevice(dev);
        if (stream) hipStreamSynchronize(stream);
        pool_release_all();
        if (co->d_tab) hipFree(co->d_tab);
        for (hipEvent_t e : co->inflight) hipEventDestroy(e);
        for (hipEvent_t e : co->free_events) hipEventDestroy(e);
        if (arena) hipFree(arena);
        if (ev0) hipEventDestroy(ev0);
        if (ev1) hipEventDestroy(ev1);
        if (stream) hipStreamDestroy(stream);
    }
    void arena_reset() { arena_used = 0; }
    // reserve the total a call needs up front (growing invalidates earlier pointers)
    int arena_reserve(size_t words) {
        if (words <= arena_words) return HE_OK;
        if (arena_frames > 0)  // (a composed call holds pointers into the arena below a step's frame: it reserved too little)
            return fail(HE_EINVAL, "internal error: a step of a composed call needs %zu words of scratch, %zu are left", words, arena_words);
        if (capturing)
            return fail(HE_EINVAL, "graph capture: the scratch arena would have to grow (run the sequence once before capturing it)");
        HIP_TRY(hipStreamSynchronize(stream));
        if (arena && live_graphs > 0) retired_arenas.push_back(arena);
        else if (arena) HIP_TRY(hipFree(arena));
        arena = nullptr;
        arena_words = 0;
        size_t want = words + words / 4;
        HIP_TRY(hipMalloc((void **)&arena, want * sizeof(uint64_t)));
        arena_words = want;
        return HE_OK;
    }
    uint64_t *arena_take(size_t words) {
        uint64_t *p = arena + arena_used;
        arena_used += (words + 1) & ~(size_t)1;  // keep 16-byte alignment
        return p;
    }
    // A step of a composed call (he_lintrans_evaluate_many) runs an entry point's launches, which reserve and take their scratch
    // as if the arena were empty: while a frame is open the arena they see starts above what the composed call has taken, and a
    // reserve that would have to grow it fails instead (arena_reserve).  Stream order makes a closed frame's scratch free for the
    // next one.
    int arena_frames = 0;
    struct ArenaFrame {
        Ctx &c;
        const size_t mark;
        explicit ArenaFrame(Ctx &ctx) : c(ctx), mark(ctx.arena_used) {
            c.arena += mark; c.arena_words -= mark; c.arena_used = 0; c.arena_frames++;
        }
        ~ArenaFrame() { c.arena -= mark; c.arena_words += mark; c.arena_used = mark; c.arena_frames--; }
        ArenaFrame(const ArenaFrame &) = delete;
    };
};

// a device-resident automorphism index table (N x 4 bytes), shared by every AutoIndex handle of its (ring, Galois element)
struct IndexTable {
    std::shared_ptr<Ctx> ctx;
    uint32_t *d = nullptr;
    ~IndexTable() {
        if (!d) return;
        hipSetDevice(ctx->dev);
        hipStreamSynchronize(ctx->stream);
        hipFree(d);
    }
};
struct Ring : Obj {
    std::shared_ptr<Ctx> ctx;
    // he_automorphism_index_create: tables by Galois element, built once and kept (the reference caches them the same way,
    // Evaluator.automorphismIndex, core/rlwe/evaluator.go:81-86): the drivers above the ABI create and drop index handles per use,
    // and a hipMalloc / hipFree pair per handle synchronises the device each time
    std::mutex index_mu;
    std::unordered_map<uint64_t, std::shared_ptr<IndexTable>> index_cache;
    static constexpr size_t kIndexCacheCap = 4096;
    int logN = 0, N = 0;
    int type = 0;  // 0 Standard, 1 ConjugateInvariant
    std::vector<uint64_t> moduli;
    std::vector<SubRingHost> sub;
    std::vector<std::vector<uint64_t>> rescale;  // [j-1][i]
    ModConst *d_mc = nullptr;
    uint64_t *d_twf = nullptr, *d_twi = nullptr;
    std::vector<uint8_t> small;
    double *d_twdf = nullptr, *d_twdi = nullptr;
    RingDev dev{};
    Ring() : Obj(T_RING) {}
    ~Ring() override {
        hipSetDevice(ctx->dev);
        hipStreamSynchronize(ctx->stream);
        if (d_mc) hipFree(d_mc);
        if (d_twf) hipFree(d_twf);
        if (d_twi) hipFree(d_twi);
        if (d_twdf) hipFree(d_twdf);
        if (d_twdi) hipFree(d_twdi);
    }
    int nmod() const { return (int)moduli.size(); }
};

// a captured launch sequence (he_graph_*): the instantiated hipGraph plus the buffers its nodes address that were released
// while it was being captured
struct Graph : Obj {
    std::shared_ptr<Ctx> ctx;
    hipGraphExec_t exec = nullptr;
    int nodes = 0;
    std::vector<std::pair<size_t, void *>> hold;
    Graph() : Obj(T_GRAPH) {}
    ~Graph() override {
        hipSetDevice(ctx->dev);
        if (exec) {
            hipStreamSynchronize(ctx->stream);  // a replay may still be in flight
            hipGraphExecDestroy(exec);
        }
        for (auto &b : hold) ctx->pool_give(b.first, b.second);
        if (counted) ctx->graph_released();
    }
    bool counted = false;  // this graph is included in ctx->live_graphs
};

struct Poly : Obj {
    std::shared_ptr<Ctx> ctx;
    int N = 0, nlimbs = 0, batch = 0;
    uint64_t *d = nullptr;
    Poly() : Obj(T_POLY) {}
    ~Poly() override {
        hipSetDevice(ctx->dev);
        if (d) ctx->pool_give((size_t)batch * nlimbs * N * 8, d);
    }
    View view() const { return View{d, (size_t)nlimbs * N}; }
    View view_at(int limb) const { return View{d + (size_t)limb * N, (size_t)nlimbs * N}; }
};

struct AutoIndex : Obj {
    std::shared_ptr<Ctx> ctx;
    int N = 0;
    uint64_t gal = 0;
    std::shared_ptr<IndexTable> tab;  // owns the device memory (shared through the ring's cache)
    uint32_t *d = nullptr;            // = tab->d
    AutoIndex() : Obj(T_INDEX) {}
};

// constant pool: host vectors concatenated into one device buffer
struct ConstPool {
    std::vector<uint64_t> host;
    uint64_t *dev = nullptr;
    size_t add(const std::vector<uint64_t> &v) {
        size_t off = host.size();
        host.insert(host.end(), v.begin(), v.end());
        return off;
    }
    int upload() {
        if (host.empty()) return HE_OK;
        HIP_TRY(hipMalloc((void **)&dev, host.size() * sizeof(uint64_t)));
        HIP_TRY(hipMemcpy(dev, host.data(), host.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
        return HE_OK;
    }
    void release() {
        if (dev) hipFree(dev);
        dev = nullptr;
    }
};
struct ModUpRef {
    int nsrc = 0, ndst = 0;
    size_t a = 0, T = 0, vt = 0, Td = 0, vtd = 0, fc = 0, t60 = 0;
    const uint64_t *fc_on(const ConstPool &p) const { return p.dev + fc; }
    const uint64_t *t60_on(const ConstPool &p) const { return p.dev + t60; }
    ModUpDev on(const ConstPool &p) const { return ModUpDev{nsrc, ndst, p.dev + a, p.dev + T, p.dev + vt}; }
    const double *Td_on(const ConstPool &p) const { return reinterpret_cast<const double *>(p.dev + Td); }
    const double *vtd_on(const ConstPool &p) const { return reinterpret_cast<const double *>(p.dev + vtd); }
};
static uint64_t dbits(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }
static ModUpRef pool_modup(ConstPool &pool, const std::vector<uint64_t> &S, const std::vector<uint64_t> &D) {
    ModUpHost h = build_modup_constants(S, D);
    ModUpRef r;
    r.nsrc = h.nsrc; r.ndst = h.ndst;
    r.a = pool.add(h.a); r.T = pool.add(h.T); r.vt = pool.add(h.vt);
    // double-precision copies for the destination moduli the f64 path handles (plain, non-Montgomery integers)
    std::vector<uint64_t> Td((size_t)h.ndst * h.nsrc * 2, 0), vtd((size_t)h.ndst * (h.nsrc + 1), 0);
    for (int j = 0; j < h.ndst; j++) {
        const uint64_t p = D[j];
        if (p >> 47) continue;
        const uint64_t rinv = invmod(to_mont(1, p), p);  // 2^-64 mod p
        for (int i = 0; i < h.nsrc; i++) {
            const uint64_t t = mulmod(h.T[(size_t)j * h.nsrc + i], rinv, p);
            Td[((size_t)j * h.nsrc + i) * 2] = dbits((double)t);
            Td[((size_t)j * h.nsrc + i) * 2 + 1] = dbits((double)mulmod(t, (1ull << kYSplitBits) % p, p));
        }
        for (int v = 0; v <= h.nsrc; v++) vtd[(size_t)j * (h.nsrc + 1) + v] = dbits((double)h.vt[(size_t)j * (h.nsrc + 1) + v]);
    }
    r.Td = pool.add(Td); r.vtd = pool.add(vtd);
    // lean integer path of the fused kernel: per destination {vt[1] 2^64 mod p, (p - floor(prod(S)/2) mod p) 2^64 mod p}
    std::vector<uint64_t> fc((size_t)h.ndst * 2, 0);
    for (int j = 0; j < h.ndst; j++) {
        const uint64_t p = D[j];
        fc[2 * j] = to_mont(h.vt[(size_t)j * (h.nsrc + 1) + 1], p);
        fc[2 * j + 1] = to_mont((p - half_product_mod(S, p)) % p, p);
    }
    r.fc = pool.add(fc);
    // the same lean path with its sum reduced at radix 2^30 (R = 2^60, see modup_fused_kernel): per destination
    // {T[i] 2^60 mod p ..., vt[1] 2^60 mod p, (p - floor(prod(S)/2) mod p) 2^60 mod p}
    std::vector<uint64_t> t60((size_t)h.ndst * (h.nsrc + 2), 0);
    for (int j = 0; j < h.ndst; j++) {
        const uint64_t p = D[j];
        const uint64_t rinv = invmod(to_mont(1, p), p);  // 2^-64 mod p
        auto m60 = [&](uint64_t x) { return (uint64_t)(((u128)(x % p) << 60) % p); };
        for (int i = 0; i < h.nsrc; i++) t60[(size_t)j * (h.nsrc + 2) + i] = m60(mulmod(h.T[(size_t)j * h.nsrc + i], rinv, p));
        t60[(size_t)j * (h.nsrc + 2) + h.nsrc] = m60(h.vt[(size_t)j * (h.nsrc + 1) + 1]);
        t60[(size_t)j * (h.nsrc + 2) + h.nsrc + 1] = m60((p - half_product_mod(S, p)) % p);
    }
    r.t60 = pool.add(t60);
    return r;
}

// ring.BasisExtender (ring/basis_extension.go:14-89) over a combined QP modulus table:
// modulus index i < LQ -> Q[i], LQ + j -> P[j].
struct BasisExtender : Obj {
    std::shared_ptr<Ctx> ctx;
    std::shared_ptr<Ring> Q, P;
    int LQ = 0, LP = 0;
    int type = 0;  // ring type of Q and P: 0 Standard, 1 ConjugateInvariant (NTTs fold around the standard network, no fused plans)
    ModConst *d_mc = nullptr;
    uint64_t *d_twf = nullptr, *d_twi = nullptr;
    std::vector<uint8_t> small;
    double *d_twdf = nullptr, *d_twdi = nullptr;
    uint64_t *d_tws = nullptr;
    RingDev qp{};
    ConstPool pool;
    std::vector<ModUpRef> qtop, ptoq;                      // per source level
    std::vector<std::vector<uint64_t>> md_ptoq, md_qtop;   // modDownConstants [levelP][i], [levelQ][j]
    BasisExtender() : Obj(T_BE) {}
    ~BasisExtender() override {
        hipSetDevice(ctx->dev);
        hipStreamSynchronize(ctx->stream);
        if (d_mc) hipFree(d_mc);
        if (d_twf) hipFree(d_twf);
        if (d_twi) hipFree(d_twi);
        if (d_twdf) hipFree(d_twdf);
        if (d_twdi) hipFree(d_twdi);
        if (d_tws) hipFree(d_tws);
        pool.release();
    }
    uint64_t modulus(int idx) const { return idx < LQ ? Q->moduli[idx] : P->moduli[idx - LQ]; }
};

// closed-form multiply counts of one primitive call (per batch entry), see Ctx::alg_valu
struct Valu {
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    int logN, N;
    explicit Valu(int logN_) : logN(logN_), N(1 << logN_) {}
    void mul(bool f64, double per_coeff) { v[f64 ? 1 : 0] += per_coeff * N; }
    void ntt(bool f64, double n = 1.0) {  // (N/2) logN butterflies + N (N^-1 / the final reduction), SURVEY.md section 8(d)
        v[f64 ? 1 : 0] += n * (0.5 * logN + 1.0) * N;
        v[f64 ? 3 : 2] += n * 0.5 * logN * N;
    }
    void into(Ctx &c, int batch) const { for (int i = 0; i < 4; i++) c.alg_valu[i] += v[i] * batch; }
};
inline bool cls_f64(const std::vector<uint8_t> &small, int idx) { return small[(size_t)idx] == 2; }
// ModUp source -> destination: y_i per source limb, |src| products per destination limb
inline void valu_modup(Valu &V, const std::vector<uint8_t> &small, int s0, int ns, const std::vector<int> &dst) {
    for (int i = 0; i < ns; i++) V.mul(cls_f64(small, s0 + i), 1.0);
    for (int j : dst) V.mul(cls_f64(small, j), (double)ns);
}
// ModDownQPtoQNTT of one polynomial: INTT of the P part, ModUpPtoQ, NTT of the extension, the last product per Q limb
inline void valu_moddown(Valu &V, const BasisExtender &be, int levelQ, int levelP, bool ntt_domain = true) {
    std::vector<int> dq;
    for (int i = 0; i <= levelQ; i++) dq.push_back(i);
    if (ntt_domain) for (int j = 0; j <= levelP; j++) V.ntt(cls_f64(be.small, be.LQ + j));
    valu_modup(V, be.small, be.LQ, levelP + 1, dq);
    for (int i = 0; i <= levelQ; i++) { if (ntt_domain) V.ntt(cls_f64(be.small, i)); V.mul(cls_f64(be.small, i), 1.0); }
}
// DecomposeNTT (with_intt: the inverse transform of the input) and / or the key inner product over beta digits
inline void valu_keyswitch(Valu &V, const BasisExtender &be, int levelQ, int levelP, int beta, bool decompose, bool inner) {
    const int alpha = levelP + 1;
    if (decompose) {
        for (int i = 0; i <= levelQ; i++) V.ntt(cls_f64(be.small, i));
        for (int d = 0; d < beta; d++) {
            const int s0 = d * alpha, e0 = std::min(s0 + alpha, levelQ + 1);
            std::vector<int> dst;
            for (int i = 0; i <= levelQ; i++) if (i < s0 || i >= e0) dst.push_back(i);
            for (int j = 0; j <= levelP; j++) dst.push_back(be.LQ + j);
            valu_modup(V, be.small, s0, e0 - s0, dst);
            for (int j : dst) V.ntt(cls_f64(be.small, j));
        }
    }
    if (inner) {
        for (int i = 0; i <= levelQ; i++) V.mul(cls_f64(be.small, i), 2.0 * beta);
        for (int j = 0; j <= levelP; j++) V.mul(cls_f64(be.small, be.LQ + j), 2.0 * beta);
    }
}
// GadgetProduct = DecomposeNTT + inner product + ModDown of both components
inline void valu_gadget_product(Valu &V, const BasisExtender &be, int levelQ, int levelP, int beta, bool decompose) {
    valu_keyswitch(V, be, levelQ, levelP, beta, decompose, true);
    if (levelP >= 0) { valu_moddown(V, be, levelQ, levelP); valu_moddown(V, be, levelQ, levelP); }
}

// rlwe.Evaluator hot path: BasisExtender + ring.Decomposer constants (ring/basis_extension.go:320-377)
// descriptors of the fused basis-extension kernel, grouped by source-limb count
struct FusedGroup {
    ModUpDesc *dev;
    int n, nsrc;
    int dst_classes;  // bit 0: some destination modulus >= 2^47, bit 1: some below
    int total_limbs;  // source + destination limbs over the group's descriptors
};
struct FusedPlan {
    bool ok = false;
    std::vector<FusedGroup> groups;
};
struct Poly;
struct Evk;
struct Evaluator : Obj {
    std::shared_ptr<BasisExtender> be;
    ConstPool pool;
    // automorphism index tables by Galois element, built on first use and kept (the reference caches them the same way:
    // Evaluator.automorphismIndex, core/rlwe/evaluator.go:81-86,:190-205); N x 4 bytes each
    std::unordered_map<uint64_t, uint32_t *> auto_index;
    static constexpr size_t kAutoIndexCap = 4096;
    // dec[nbPi-2][digit][j]: source = first j+2 limbs of the digit, target = all Q then P[:nbPi]
    std::vector<std::vector<std::vector<ModUpRef>>> dec;
    std::map<std::tuple<int, int, int>, FusedPlan> dec_plans;  // (levelQ, levelP, nbPi)
    std::map<std::pair<int, int>, FusedPlan> md_plans;         // (levelQ, levelP)
    std::vector<ModUpDesc *> plan_mem;
    Evaluator() : Obj(T_EVAL) {}
    ~Evaluator() override {
        hipSetDevice(be->ctx->dev);
        hipStreamSynchronize(be->ctx->stream);
        for (ModUpDesc *p : plan_mem) hipFree(p);
        for (auto &kv : auto_index) hipFree(kv.second);
        pool.release();
    }
};

// GadgetCiphertext on the device: [beta][2][nQk + nPk][N], Q limbs then P limbs per (d,k)
struct Evk : Obj {
    std::shared_ptr<Evaluator> ev;
    int beta = 0, nQk = 0, nPk = 0;
    int pw2 = 0;                 // BaseTwoDecomposition
    std::vector<int> nj, prefix; // bit windows per RNS digit and their prefix sums (pw2 != 0)
    double *keyd = nullptr;      // plain key words as doubles for the limbs below 2^47 (fused NTT+MAC kernel): the blocks of d,
                                 // each row of 4096 / 8192 coefficients permuted for that kernel (launch_key_to_f64)
    uint64_t *d = nullptr;
    // the key's words lie below word_mul * q: 1 for words as created or committed (canonical), raised by the lazy helpers of
    // hering_rgsw.h and set back by HE_RGSW_REDUCE; saturates at kWordMulCap, which stands for "no bound is known"
    uint64_t word_mul = 1;
    static constexpr uint64_t kWordMulCap = (uint64_t)1 << 32;
    Evk() : Obj(T_EVK) {}
    // the key as a batch of 2 beta rows (digit d, component c at 2 d + c) of nQk + nPk limbs
    View rows() const { return View{d, (size_t)(nQk + nPk) * ev->be->Q->N}; }
    ~Evk() override {
        hipSetDevice(ev->be->ctx->dev);
        hipStreamSynchronize(ev->be->ctx->stream);
        if (d) hipFree(d);
        if (keyd) hipFree(keyd);
    }
};

// BuffDecompQP: [batch][beta_max][LQ + LP][N]
struct Decomp : Obj {
    std::shared_ptr<Evaluator> ev;
    int batch = 0, beta_max = 0, width = 0;  // width = LQ + LP limbs per digit
    // what the buffer currently holds: levels of the last he_decompose_ntt / he_decomp_fill (-1: nothing yet)
    int fillQ = -1, fillP = -1, fill_beta = 0;
    uint64_t *d = nullptr;
    Decomp() : Obj(T_DECOMP) {}
    ~Decomp() override {
        hipSetDevice(ev->be->ctx->dev);
        if (d) ev->be->ctx->pool_give((size_t)batch * bstride() * 8, d);
    }
    size_t bstride() const { return (size_t)beta_max * width * ev->be->Q->N; }
    View view() const { return View{d, bstride()}; }
    size_t dstride() const { return (size_t)width * ev->be->Q->N; }
};

// The handle registry: every entry point looks its handles up (six to ten per call), from as many threads as there are callers.
// One mutex made those look-ups queue behind each other (64 callers: the queue's dispatcher sat idle while the callers fought for
// this lock); 64 shards by handle, readers share a shard's lock.
struct RegShard {
    std::shared_mutex mu;
    std::unordered_map<uint64_t, std::shared_ptr<Obj>> m;
};
RegShard g_reg[64];
std::atomic<uint64_t> g_next{0x1000};
inline RegShard &reg_shard(uint64_t h) { return g_reg[h & 63]; }

uint64_t reg(std::shared_ptr<Obj> o) {
    const uint64_t h = g_next.fetch_add(1, std::memory_order_relaxed);
    RegShard &sh = reg_shard(h);
    std::unique_lock<std::shared_mutex> l(sh.mu);
    sh.m[h] = std::move(o);
    return h;
}
template <class T>
std::shared_ptr<T> get(uint64_t h, ObjType t) {
    RegShard &sh = reg_shard(h);
    std::shared_lock<std::shared_mutex> l(sh.mu);
    auto it = sh.m.find(h);
    if (it == sh.m.end() || it->second->type != t) return nullptr;
    return std::static_pointer_cast<T>(it->second);
}
void reg_drop(uint64_t h) {  // forget a handle whatever it names (an object that changes owner)
    RegShard &sh = reg_shard(h);
    std::unique_lock<std::shared_mutex> l(sh.mu);
    sh.m.erase(h);
}
int unreg(uint64_t h, ObjType t) {
    std::shared_ptr<Obj> keep;
    {
        RegShard &sh = reg_shard(h);
        std::unique_lock<std::shared_mutex> l(sh.mu);
        auto it = sh.m.find(h);
        if (it == sh.m.end() || it->second->type != t) return fail(HE_EHANDLE, "unknown handle %llu", (unsigned long long)h);
        keep = it->second;
        sh.m.erase(it);
    }
    keep.reset();
    return HE_OK;
}
#define GET(var, T, h, tag)                                                                          \
    auto var = get<T>(h, tag);                                                                       \
    if (!var) return fail(HE_EHANDLE, "%s: bad %s handle %llu", __func__, #T, (unsigned long long)(h))

void co_flush_mine(Ctx &ctx);
struct NoFlush {};
struct Scope {  // per-call: select device, lock the context, reset the scratch arena
    Ctx *c;
    // Deferred submission: launches made directly (batched handles, transfers, key uploads ...) must come after the calling
    // thread's own pending requests -- wait for those first (BEFORE the context's lock: the dispatcher launches under it).
    explicit Scope(Ctx *ctx) : c(ctx) {
        if (c->co->depth.load(std::memory_order_relaxed) > 0 && !g_dispatcher_thread) co_flush_mine(*c);
        c->mu.lock();
        hipSetDevice(c->dev);
        c->arena_reset();
    }
    // (a launch that touches nothing a pending request can address: the zero fill of a buffer fresh from the pool)
    Scope(Ctx *ctx, NoFlush) : c(ctx) {
        c->mu.lock();
        hipSetDevice(c->dev);
        c->arena_reset();
    }
    ~Scope() { c->mu.unlock(); }
};
// host words into scratch from kernel arguments (no host buffer outlives the call; a captured graph holds them)
template <class T>
int scratch_words(Ctx &ctx, const std::vector<size_t> &w, T **d) {
    TRY(ctx.arena_reserve(w.size() + 2));
    size_t *p = reinterpret_cast<size_t *>(ctx.arena_take(w.size()));
    *d = reinterpret_cast<T *>(p);
    HIP_TRY(launch_tab_fill(p, w.data(), (int)w.size(), ctx.stream));
    return HE_OK;
}
// a host selection of key indices on the device, two int32 per word
int scratch_selection(Ctx &ctx, const int32_t *sel, size_t n, const int32_t **d) {
    std::vector<size_t> tab((n + 1) / 2, 0);
    for (size_t i = 0; i < n; i++) tab[i / 2] |= (size_t)(uint32_t)sel[i] << (32 * (i & 1));
    return scratch_words(ctx, tab, d);
}

// ---- the context's submission queue (struct Coalescer): coalescing of concurrent single-ciphertext calls ---------------------
constexpr size_t kTabRowsMin = 16;  // rows of the entry table reserved per batch entry (he_ctx_set_coalescing sizes it)
int co_inflight(Coalescer &c) {  // batches still running or queued on the device (caller holds c.mu)
    while (!c.inflight.empty() && hipEventQuery(c.inflight.front()) == hipSuccess) {
        if (!c.inflight_begin.empty()) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, c.inflight_begin.front(), c.inflight.front()) == hipSuccess) c.dbg[12] += (uint64_t)(ms * 1000.f);
            c.free_events.push_back(c.inflight_begin.front());
            c.inflight_begin.pop_front();
        }
        c.free_events.push_back(c.inflight.front());
        c.inflight.pop_front();
    }
    (void)hipGetLastError();  // hipErrorNotReady is not an error here
    return (int)c.inflight.size();
}
// the launches of `batch` (all of one key): one batched launch sequence over entry tables where the shape allows, one call per
// request otherwise.  Fills every request's own status / message; returns the number of requests served one by one.
int co_run(Ctx &ctx, Coalescer &c, const std::vector<CoReq *> &batch, hipEvent_t done_ev) {
    CoReq &r0 = *batch[0];
    const int R = (int)batch.size();
    int B = 0;  // entries: a request over handles of batch nb contributes nb of them
    for (const CoReq *r : batch) B += r->nb;
    const size_t ns = r0.ops.size();
    Scope sc(&ctx);
    if (r0.op >= 0 && r0.op < 32) { c.op_launches[r0.op]++; c.op_calls[r0.op] += (uint64_t)R; }  // (under the context's lock, as its reader)
    bool tables = R > 1;
    int rc = HE_OK;
    if (tables && r0.tables_ok) rc = r0.tables_ok(&tables);
    if (rc == HE_OK && tables && ns * (size_t)B > c.tab_words) tables = false;  // (gathered under a larger max_batch than the table was sized for)
    // an operand present in one request and absent in another cannot share a table row (the key fixes the count, not the nulls)
    for (int z = 1; tables && z < R; z++)
        for (size_t s = 0; s < ns; s++) tables = tables && (batch[z]->ops[s].p == nullptr) == (r0.ops[s].p == nullptr);
    int fallback = 0;
    if (rc != HE_OK) {
        const std::string msg = g_err;
        for (CoReq *r : batch) { r->rc = rc; r->err = msg; }
    } else if (R == 1 || !tables) {
        // one request, or a shape whose pipeline has launches without entry tables (unfused ModDown, conjugate-invariant rings,
        // base-2 gadgets): one call per request, each with its own status
        if (R > 1) fallback = R;
        for (CoReq *r : batch) {
            ctx.arena_reset();
            r->rc = r->run(r->ops.data(), r->nb);
            if (r->rc != HE_OK) r->err = g_err;
        }
    } else {
        // entry tables: row s of the table holds, per entry, the word offset of that entry's operand s from entry 0's
        std::vector<size_t> vals(ns * (size_t)B, 0);
        std::vector<View> v(ns);
        for (size_t s = 0; s < ns; s++) {
            uint64_t *base = r0.ops[s].p;
            if (!base) continue;
            int e = 0;
            for (const CoReq *r : batch)
                for (int i = 0; i < r->nb; i++, e++) vals[s * B + e] = (size_t)(r->ops[s].p + (size_t)i * r->ops[s].bstride - base);
        }
        // a slot that already holds these offsets, or the least recently used one
        int slot = -1, lru = 0;
        for (int i = 0; i < Coalescer::kTabSlots; i++) {
            if (c.tab_slot[i].vals == vals) { slot = i; break; }
            if (c.tab_slot[i].used < c.tab_slot[lru].used) lru = i;
        }
        hipError_t e = hipSuccess;
        if (slot < 0) {
            slot = lru;
            e = launch_tab_fill(c.d_tab + (size_t)slot * c.tab_words, vals.data(), (int)vals.size(), ctx.stream);
            if (e == hipSuccess) { c.tab_slot[slot].vals = vals; c.tab_fills++; }
            else c.tab_slot[slot].vals.clear();
        } else c.tab_hits++;
        c.tab_slot[slot].used = ++c.tab_clock;
        size_t *tab = c.d_tab + (size_t)slot * c.tab_words;
        for (size_t s = 0; s < ns; s++) v[s] = r0.ops[s].p ? View{r0.ops[s].p, 0, tab + s * B} : View{nullptr, 0};
        if (e != hipSuccess) rc = fail(HE_EDEVICE, "launch_tab_fill: %s", hipGetErrorString(e));
        else rc = r0.run(v.data(), B);
        const std::string msg = rc ? g_err : std::string();
        for (CoReq *r : batch) { r->rc = rc; r->err = msg; }
    }
    if (done_ev && hipEventRecord(done_ev, ctx.stream) != hipSuccess) (void)hipGetLastError();
    return fallback;
}
// the calling thread is the leader: serve batches until its own request is done (caller holds lk on c.mu)
void co_wake_all(Coalescer &c) {
    c.gen.fetch_add(1, std::memory_order_release);
    syscall(SYS_futex, reinterpret_cast<uint32_t *>(&c.gen), FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
}
// `extra` (optional): the other requests of the calling thread (co_submit_many): it leads until ALL of its requests are done
void co_lead(Ctx &ctx, Coalescer &c, std::unique_lock<std::mutex> &lk, CoReq &mine, const std::vector<CoReq *> *extra = nullptr) {
    using clock = std::chrono::steady_clock;
    hipSetDevice(ctx.dev);
    auto all_done = [&]() -> bool {
        if (!mine.done.load(std::memory_order_acquire)) return false;
        if (extra) for (CoReq *r : *extra) if (!r->done.load(std::memory_order_acquire)) return false;
        return true;
    };
    while (!all_done()) {
        // gather: up to max_batch requests.  While the device still has two batches of this queue ahead of it, waiting is free.
        // Otherwise stop once no request has arrived for window_us AND at least half of the recent batches' callers are here
        // (callers that wait for their result come back together, as fast as the OS schedules them), or 8 window_us after the
        // oldest request arrived.  No window at all for a lone caller (crowd == 0).
        // (at least one: a request that passed the "queue on?" test just before the queue was switched off is still served)
        const int max_batch = std::max(1, c.max_batch.load(std::memory_order_relaxed));
        const auto g0 = clock::now();
        for (;;) {
            if ((int)c.pending.size() >= max_batch) { c.dbg[2]++; break; }
            const bool busy = co_inflight(c) >= 2;
            const auto now = clock::now();
            const auto waited = std::chrono::duration_cast<std::chrono::microseconds>(now - c.pending.front()->arrived).count();
            const long long win = c.crowd > 0 ? c.window_us : 0;
            // Round 5: the rule counts CALLERS.  Every thread that filed a request in the last few milliseconds is expected back
            // (callers of the one-ciphertext interface run the same circuit: they arrive at the same operation one after the
            // other); once all of them are waiting here -- for this operation or another -- nobody else can arrive and waiting
            // is pointless; until then the leader waits, at most 8 windows from the oldest request's arrival.
            int active = 0, here = 0;
            {
                uint64_t ids[256];
                for (auto it = c.seen.begin(); it != c.seen.end();) {
                    if (std::chrono::duration_cast<std::chrono::microseconds>(now - it->second).count() > 3000 + 8 * win) it = c.seen.erase(it);
                    else { ++active; ++it; }
                }
                for (const CoReq *r : c.pending) {
                    bool dup = false;
                    for (int i = 0; i < here && i < 256; i++) dup = dup || ids[i] == r->caller;
                    if (!dup) { if (here < 256) ids[here] = r->caller; here++; }
                }
            }
            if (!busy && (here >= active || waited >= 8 * win)) {
                c.dbg[here >= active ? 0 : 1]++; c.dbg[5] += (uint64_t)here; c.dbg[6] += (uint64_t)active;
                break;
            }
            if (busy) {
                c.cv_leader.wait_for(lk, std::chrono::microseconds(100));  // arrivals notify
            } else {  // a few microseconds: a timed futex wait would oversleep by the timer slack
                lk.unlock();
                sched_yield();
                lk.lock();
            }
        }
        std::vector<CoReq *> batch;
        // Which operation goes first: the oldest request's -- unless a caller of the same cohort is BEHIND it.  Callers of the
        // one-ciphertext interface that run the same circuit (b.RunParallel) make the same sequence of calls, so a thread's call
        // count is its position in the circuit; once two groups of callers have drifted apart (a timeout, a slow wake-up) they
        // would stay apart for ever, each group's batches a fraction of what they could be.  Serving the group that is behind
        // (fewer calls made, within 64 calls of the oldest request's thread: unrelated threads keep arrival order) lets it catch
        // up with the group that waits here, and the two merge.
        const CoReq *hp = c.pending.front();
        for (const CoReq *r : c.pending)
            if (r->seq < hp->seq && c.pending.front()->seq - r->seq <= 64) hp = r;
        const CoReq &head = *hp;
        int entries = 0;
        for (auto it = c.pending.begin(); it != c.pending.end();) {
            if ((*it)->same_key(head) && (batch.empty() || entries + (*it)->nb <= max_batch)) { entries += (*it)->nb; batch.push_back(*it); it = c.pending.erase(it); }
            else ++it;
        }
        if (batch.size() > 1 || !c.pending.empty()) c.crowd = 256;
        else if (c.crowd > 0) c.crowd--;
        c.recent[c.n_launches & 3] = (int)batch.size();
        // the completion event feeds the "two batches ahead" test of the gathering loop: not needed for a lone caller, whose
        // stream drain would otherwise also wait for the event's barrier packet (a third of a single-ciphertext call's latency)
        hipEvent_t e = nullptr;
        if (c.crowd > 0) {
            if (!c.free_events.empty()) { e = c.free_events.back(); c.free_events.pop_back(); }
            else if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) e = nullptr;
        }
        if (batch[0]->op != CO_ZERO) { c.n_calls += batch.size(); c.n_launches++; c.n_max = std::max<uint64_t>(c.n_max, batch.size()); }  // (operator calls: not the zero fills of allocations)
        const auto g1 = clock::now();
        c.dbg[3] += (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(g1 - g0).count();
        lk.unlock();
        const int fallback = co_run(ctx, c, batch, e);
        const uint64_t run_us = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(clock::now() - g1).count();
        // (status and message were written by co_run; `done` is the last touch: the owner may leave at once)
        bool mine_in_batch = false;
        for (CoReq *r : batch) {
            if (r == &mine || (extra && std::find(extra->begin(), extra->end(), r) != extra->end())) { mine_in_batch = true; continue; }
            r->done.store(true, std::memory_order_release);
        }
        co_wake_all(c);
        lk.lock();
        c.dbg[4] += run_us;
        c.n_fallback += (uint64_t)fallback;
        if (e) c.inflight.push_back(e);
        if (mine_in_batch)
            for (CoReq *r : batch)
                if (r == &mine || (extra && std::find(extra->begin(), extra->end(), r) != extra->end())) r->done.store(true, std::memory_order_release);
    }
}
// files the requests of ONE call (most calls: one; the polynomials of a ciphertext in he_rescale_ct: several, which then share
// a batch) and returns when all of them have been enqueued on the stream
uint64_t co_me() {
    static std::atomic<uint64_t> next_caller{1};
    thread_local uint64_t me = next_caller.fetch_add(1, std::memory_order_relaxed);
    return me;
}
thread_local uint64_t g_my_calls = 0;  // queued calls this thread has made: its position in the circuit (see co_lead)
void co_note_caller(Coalescer &c, uint64_t me, std::chrono::steady_clock::time_point now) {
    for (auto &sv : c.seen) if (sv.first == me) { sv.second = now; return; }
    c.seen.emplace_back(me, now);
}
void co_sleep(Coalescer &c, uint32_t g) {  // until the generation word moves on from g
    c.sleepers.fetch_add(1, std::memory_order_seq_cst);
    if (c.gen.load(std::memory_order_seq_cst) == g)
        syscall(SYS_futex, reinterpret_cast<uint32_t *>(&c.gen), FUTEX_WAIT_PRIVATE, g, nullptr, nullptr, 0);
    c.sleepers.fetch_sub(1, std::memory_order_acq_rel);
}

// ---- deferred submission -------------------------------------------------------------------------------------------------------
// The blocking queue above costs every call two thread hand-overs (caller -> leader -> caller) that the device waits out: with 16
// callers replaying a bootstrapping circuit a queue round took ~400 us of host time for ~260 us of kernels.  Deferred: the call
// files a heap copy of its request and returns HE_OK; the context's dispatcher thread gathers the FIRST pending call of every
// thread (a thread's calls launch in the order it made them), batches the ones that share a key and launches.  Callers run ahead
// of the device by at most `depth` requests.  What a deferred call can no longer report -- a launch that fails after the
// arguments were accepted -- is kept and returned by the next he_ctx_sync.  Everything that launches directly (batched handles,
// transfers, graph capture) first waits for the calling thread's pending requests (Scope); he_ctx_sync waits for every request
// filed before it.  Data handed from one thread to another needs a he_ctx_sync in between (in the blocking mode a returned call
// was already in stream order).
CoReq *co_heap_copy(CoReq &q) {
    CoReq *h = new CoReq();
    h->op = q.op; h->obj = q.obj; h->key = q.key; h->nb = q.nb;
    memcpy(h->par, q.par, sizeof h->par);
    h->blob = std::move(q.blob); h->ops = std::move(q.ops); h->keep = std::move(q.keep);
    h->run = std::move(q.run); h->tables_ok = std::move(q.tables_ok);
    return h;
}
int64_t co_now_us() { return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// the calling thread's record in this queue (create: register it on first use; nullptr when there is none / no room).
// Threads cache the pointer; a thread that ends frees its records (unless requests are still pending) for the next new thread.
struct CallerCache {
    struct Slot { uint64_t uid; Coalescer::Caller *st; };
    Slot slot[4] = {{0, nullptr}, {0, nullptr}, {0, nullptr}, {0, nullptr}};
    std::vector<Slot> all;  // every record this thread owns
    int next = 0;
    ~CallerCache() {
        std::lock_guard<std::mutex> lk(Coalescer::live_mu());  // (a queue cannot be destroyed while its record is being released)
        for (const Slot &sl : all) {
            if (!Coalescer::live().count(sl.uid)) continue;
            std::lock_guard<std::mutex> q(sl.st->mu);
            if (sl.st->pending.load(std::memory_order_seq_cst) == 0 && sl.st->q.empty()) sl.st->id.store(0, std::memory_order_release);
        }
    }
};
thread_local CallerCache g_caller_cache;
Coalescer::Caller *co_my_caller(Coalescer &c, bool create) {
    CallerCache &cc = g_caller_cache;
    for (const CallerCache::Slot &sl : cc.slot) if (sl.uid == c.uid) return sl.st;
    for (const CallerCache::Slot &sl : cc.all) if (sl.uid == c.uid) return sl.st;
    if (!create) return nullptr;
    const uint64_t me = co_me();
    Coalescer::Caller *st = nullptr;
    const int n = c.n_callers.load(std::memory_order_acquire);
    for (int i = 0; i < n && !st; i++) {  // a record a thread that ended left behind
        Coalescer::Caller *m = c.callers[i].load(std::memory_order_acquire);
        uint64_t free_id = 0;
        if (m && m->id.load(std::memory_order_relaxed) == 0 && m->id.compare_exchange_strong(free_id, me, std::memory_order_acq_rel)) st = m;
    }
    if (!st) {
        std::lock_guard<std::mutex> lk(c.mu);  // (registration: once per thread)
        const int k = c.n_callers.load(std::memory_order_relaxed);
        if (k >= Coalescer::kMaxCallers) return nullptr;
        st = new Coalescer::Caller();
        st->id.store(me, std::memory_order_relaxed);
        c.callers[k].store(st, std::memory_order_release);
        c.n_callers.store(k + 1, std::memory_order_release);
    }
    cc.slot[cc.next] = CallerCache::Slot{c.uid, st};
    cc.next = (cc.next + 1) & 3;
    cc.all.push_back(CallerCache::Slot{c.uid, st});
    return st;
}
void co_kick_dispatcher(Coalescer &c) {
    c.work.fetch_add(1, std::memory_order_seq_cst);
    if (c.disp_idle.load(std::memory_order_seq_cst))
        syscall(SYS_futex, reinterpret_cast<uint32_t *>(&c.work), FUTEX_WAKE_PRIVATE, 1, nullptr, nullptr, 0);
}
int co_defer(Ctx &ctx, const std::vector<CoReq *> &rs) {
    Coalescer &c = *ctx.co;
    Coalescer::Caller *stp = co_my_caller(c, true);
    if (!stp) return -2;  // (more live threads than records: launched directly)
    Coalescer::Caller &st = *stp;
    int depth = c.depth.load(std::memory_order_relaxed);
    if (depth > 0 && st.pending.load(std::memory_order_relaxed) >= depth) {
        // a full pipeline: sleep until HALF of it has been launched (one wake-up per depth / 2 requests, not one per call); the
        // dispatcher wakes the sleepers whose count reached the mark
        st.wait_low.store(true, std::memory_order_seq_cst);
        for (;;) {
            const uint32_t g = c.gen.load(std::memory_order_seq_cst);
            depth = c.depth.load(std::memory_order_relaxed);
            if (depth <= 0 || st.pending.load(std::memory_order_seq_cst) <= depth / 2) break;
            co_sleep(c, g);
        }
        st.wait_low.store(false, std::memory_order_seq_cst);
    }
    std::shared_lock<std::shared_mutex> alive(c.life);  // (deferred mode cannot end between this test and the push)
    if (c.depth.load(std::memory_order_relaxed) <= 0 || c.stop.load(std::memory_order_relaxed)) return -1;
    const auto now = std::chrono::steady_clock::now();
    const int n = (int)rs.size();
    CoReq *heap[16];
    std::vector<CoReq *> more;
    if (n > 16) more.resize((size_t)n);
    CoReq **hp = n > 16 ? more.data() : heap;
    for (int i = 0; i < n; i++) {
        hp[i] = co_heap_copy(*rs[i]);
        hp[i]->arrived = now; hp[i]->caller = st.id.load(std::memory_order_relaxed); hp[i]->seq = g_my_calls;
    }
    g_my_calls++;
    st.pending.fetch_add(n, std::memory_order_seq_cst);
    {
        std::lock_guard<std::mutex> lk(st.mu);
        for (int i = 0; i < n; i++) {
            hp[i]->ticket = c.next_ticket.fetch_add(1, std::memory_order_relaxed);  // (under the record's lock: increasing along its queue)
            st.q.push_back(hp[i]);
        }
    }
    st.last_us.store(co_now_us(), std::memory_order_relaxed);
    c.n_deferred.fetch_add(n, std::memory_order_seq_cst);
    co_kick_dispatcher(c);
    return HE_OK;
}
// wait until the calling thread has nothing pending
void co_flush_mine(Ctx &ctx) {
    Coalescer &c = *ctx.co;
    Coalescer::Caller *st = co_my_caller(c, false);
    if (!st || st->pending.load(std::memory_order_seq_cst) <= 0) return;
    c.flushers.fetch_add(1, std::memory_order_seq_cst);
    co_kick_dispatcher(c);
    for (;;) {
        const uint32_t g = c.gen.load(std::memory_order_seq_cst);
        if (st->pending.load(std::memory_order_seq_cst) <= 0) break;
        co_sleep(c, g);
    }
    c.flushers.fetch_sub(1, std::memory_order_seq_cst);
}
// wait until every request filed before this call has been launched; returns (and clears) the first deferred failure
int co_flush_filed(Ctx &ctx) {
    Coalescer &c = *ctx.co;
    const uint64_t upto = c.next_ticket.load(std::memory_order_seq_cst);  // tickets below this were filed
    auto behind = [&]() -> bool {
        if (c.launching_min.load(std::memory_order_seq_cst) < upto) return true;
        const int n = c.n_callers.load(std::memory_order_acquire);
        for (int i = 0; i < n; i++) {
            Coalescer::Caller *m = c.callers[i].load(std::memory_order_acquire);
            std::lock_guard<std::mutex> lk(m->mu);
            if (!m->q.empty() && m->q.front()->ticket < upto) return true;
        }
        // (a batch moves from the queues to `launching_min` under the records' locks, lowest ticket published first: see the dispatcher)
        return c.launching_min.load(std::memory_order_seq_cst) < upto;
    };
    if (behind()) {
        c.flushers.fetch_add(1, std::memory_order_seq_cst);
        for (;;) {
            const uint32_t g = c.gen.load(std::memory_order_seq_cst);
            if (!behind()) break;
            co_kick_dispatcher(c);
            co_sleep(c, g);
        }
        c.flushers.fetch_sub(1, std::memory_order_seq_cst);
    }
    std::unique_lock<std::mutex> lk(c.mu);
    if (c.def_rc != HE_OK) {
        const int rc = c.def_rc;
        const std::string msg = c.def_err;
        c.def_rc = HE_OK; c.def_err.clear();
        lk.unlock();
        return fail(rc, "%s (reported by a deferred call)", msg.c_str());
    }
    return HE_OK;
}
// the dispatcher thread of a context in deferred mode
void co_dispatcher_main(Ctx *ctx) {
    using clock = std::chrono::steady_clock;
    Coalescer &c = *ctx->co;
    g_dispatcher_thread = true;
    hipSetDevice(ctx->dev);
    static const bool timing = env_flag("HERING_QUEUE_TIMING");  // diagnosis: how long the device spent inside the batches
    static const int ahead_cap = std::max(2, getenv("HERING_QUEUE_AHEAD") ? atoi(getenv("HERING_QUEUE_AHEAD")) : 16);
    std::vector<CoReq *> heads, batch;
    std::vector<Coalescer::Caller *> owners;
    auto nap = [&](uint32_t seen_work, long us) {  // until a call is filed, at most `us`
        timespec ts{0, us * 1000};
        c.disp_idle.store(true, std::memory_order_seq_cst);
        if (c.work.load(std::memory_order_seq_cst) == seen_work && !c.stop.load(std::memory_order_seq_cst))
            syscall(SYS_futex, reinterpret_cast<uint32_t *>(&c.work), FUTEX_WAIT_PRIVATE, seen_work, &ts, nullptr, 0);
        c.disp_idle.store(false, std::memory_order_seq_cst);
    };
    for (;;) {
        uint32_t w = c.work.load(std::memory_order_seq_cst);
        if (c.n_deferred.load(std::memory_order_seq_cst) <= 0) {
            if (c.stop.load(std::memory_order_seq_cst)) break;  // (nothing left to launch)
            nap(w, 2000);
            continue;
        }
        const int max_batch = std::max(1, c.max_batch.load(std::memory_order_relaxed));
        const long long win = c.window_us;
        const auto g0 = clock::now();
        const CoReq *hp = nullptr;
        for (;;) {
            w = c.work.load(std::memory_order_seq_cst);
            // the candidates: every thread's first pending call (all requests of it); `oldest`: the one filed first
            heads.clear();
            int here = 0, active = 0;
            const CoReq *oldest = nullptr;
            const int64_t now_us = co_now_us();
            const int n = c.n_callers.load(std::memory_order_acquire);
            for (int i = 0; i < n; i++) {
                Coalescer::Caller *m = c.callers[i].load(std::memory_order_acquire);
                bool has = false;
                {
                    std::lock_guard<std::mutex> lk(m->mu);
                    if (!m->q.empty()) {
                        has = true;
                        const uint64_t seq = m->q.front()->seq;
                        for (CoReq *r : m->q) { if (r->seq != seq) break; heads.push_back(r); }
                        if (!oldest || m->q.front()->ticket < oldest->ticket) oldest = m->q.front();
                    }
                }
                here += has ? 1 : 0;
                // expected back: every thread that filed in the last few milliseconds (the caller-counting rule of co_lead)
                active += (has || now_us - m->last_us.load(std::memory_order_relaxed) <= 3000 + 8 * win) ? 1 : 0;
            }
            if (!oldest) break;  // (cannot happen: n_deferred > 0 and only this thread removes requests)
            // which operation: the oldest call's -- unless a thread of the same cohort is behind it (see co_lead)
            hp = oldest;
            for (const CoReq *r : heads)
                if (r->seq < hp->seq && oldest->seq - r->seq <= 64) hp = r;
            int same = 0;  // (in batch entries)
            for (const CoReq *r : heads) same += r->same_key(*hp) ? r->nb : 0;
            const auto now = clock::now();
            int ahead;
            { std::lock_guard<std::mutex> lk(c.mu); ahead = co_inflight(c); }
            const auto waited = std::chrono::duration_cast<std::chrono::microseconds>(now - oldest->arrived).count();
            if (c.stop.load(std::memory_order_relaxed)) break;
            auto spent = [&](int slot) { c.dbg[slot] += (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(clock::now() - now).count(); };
            if (ahead >= ahead_cap) { nap(w, 100); spent(8); continue; }  // far enough ahead of the device
            if (same >= max_batch) { c.dbg[2]++; break; }
            if (here >= active) { c.dbg[0]++; c.dbg[5] += (uint64_t)here; c.dbg[6] += (uint64_t)active; break; }
            if (ahead < 2 && waited >= 8 * win) { c.dbg[1]++; c.dbg[5] += (uint64_t)here; c.dbg[6] += (uint64_t)active; break; }
            if (ahead >= 2) { nap(w, 100); spent(9); }  // the device is busy: waiting is free; a filed call ends the nap
            else { sched_yield(); spent(10); }
        }
        if (!hp) continue;
        batch.clear(); owners.clear();
        int entries = 0;
        for (CoReq *r : heads)
            if (r->same_key(*hp) && (batch.empty() || entries + r->nb <= max_batch)) { entries += r->nb; batch.push_back(r); }
        uint64_t lo = UINT64_MAX;
        for (CoReq *r : batch) lo = std::min(lo, r->ticket);
        c.launching_min.store(lo, std::memory_order_seq_cst);  // (published BEFORE the requests leave their queues: he_ctx_sync never sees them nowhere)
        const int nc = c.n_callers.load(std::memory_order_acquire);
        for (CoReq *r : batch) {
            Coalescer::Caller *m = nullptr;
            for (int i = 0; i < nc && !m; i++) { Coalescer::Caller *x = c.callers[i].load(std::memory_order_acquire); if (x->id.load(std::memory_order_relaxed) == r->caller) m = x; }
            std::lock_guard<std::mutex> lk(m->mu);
            m->q.erase(std::find(m->q.begin(), m->q.end(), r));  // (one of the first few: the requests of the thread's first call)
            owners.push_back(m);
        }
        c.n_deferred.fetch_sub((int)batch.size(), std::memory_order_seq_cst);
        hipEvent_t e = nullptr, e_begin = nullptr;
        {
            std::lock_guard<std::mutex> lk(c.mu);
            auto take_event = [&]() -> hipEvent_t {
                hipEvent_t ev = nullptr;
                if (!c.free_events.empty()) { ev = c.free_events.back(); c.free_events.pop_back(); }
                else if (hipEventCreateWithFlags(&ev, timing ? hipEventDefault : hipEventDisableTiming) != hipSuccess) ev = nullptr;
                return ev;
            };
            e = take_event();
            e_begin = timing ? take_event() : nullptr;
            if (batch[0]->op != CO_ZERO) { c.n_calls += batch.size(); c.n_launches++; c.n_max = std::max<uint64_t>(c.n_max, batch.size()); }  // (operator calls: not the zero fills of allocations)
            c.dbg[11]++;
        }
        if (e_begin && hipEventRecord(e_begin, ctx->stream) != hipSuccess) (void)hipGetLastError();
        const auto g1 = clock::now();
        c.dbg[3] += (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(g1 - g0).count();
        const int fallback = co_run(*ctx, c, batch, e);
        const uint64_t run_us = (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(clock::now() - g1).count();
        {
            std::lock_guard<std::mutex> lk(c.mu);
            c.dbg[4] += run_us;
            c.n_fallback += (uint64_t)fallback;
            if (e) { c.inflight.push_back(e); if (e_begin) c.inflight_begin.push_back(e_begin); }
            for (CoReq *r : batch)
                if (r->rc != HE_OK && c.def_rc == HE_OK) { c.def_rc = r->rc; c.def_err = r->err; }
        }
        c.launching_min.store(UINT64_MAX, std::memory_order_seq_cst);
        // who has to hear about it: a thread asleep on a full pipeline whose count reached the low mark, anybody flushing.
        // (sleepers raise their flag BEFORE they read their count, this lowers the count BEFORE it reads the flag: one of the two
        // sees the other)
        const int low = c.depth.load(std::memory_order_relaxed) / 2;
        bool wake = false;
        for (Coalescer::Caller *m : owners) {
            const int left = m->pending.fetch_sub(1, std::memory_order_seq_cst) - 1;
            wake = wake || (left <= low && m->wait_low.load(std::memory_order_seq_cst));
        }
        wake = wake || c.flushers.load(std::memory_order_seq_cst) > 0;
        if (wake) {
            c.gen.fetch_add(1, std::memory_order_seq_cst);
            syscall(SYS_futex, reinterpret_cast<uint32_t *>(&c.gen), FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
        }
        for (CoReq *r : batch) delete r;  // (drops the operands' references: a released polynomial goes back to the buffer cache now)
    }
}
// stop the dispatcher (everything pending is launched first); the queue is in blocking mode afterwards
void co_stop_dispatcher(Ctx &ctx) {
    Coalescer &c = *ctx.co;
    std::thread t;
    {
        std::lock_guard<std::mutex> lk(c.mu);
        std::unique_lock<std::shared_mutex> nobody_files(c.life);  // (no call is between its "deferred?" test and its push)
        c.depth = 0;
        if (!c.dispatcher.joinable()) return;
        c.stop = true;
        t = std::move(c.dispatcher);
    }
    co_kick_dispatcher(c);
    syscall(SYS_futex, reinterpret_cast<uint32_t *>(&c.work), FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
    if (t.get_id() == std::this_thread::get_id()) t.detach();  // (cannot happen: the dispatcher never calls this)
    else t.join();
    c.stop = false;
    c.gen.fetch_add(1, std::memory_order_release);
    syscall(SYS_futex, reinterpret_cast<uint32_t *>(&c.gen), FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
}

int co_submit_many(Ctx &ctx, const std::vector<CoReq *> &rs) {
    Coalescer &c = *ctx.co;
    CoReq &r = *rs[0];
    auto all_done = [&]() -> bool {
        for (CoReq *q : rs) if (!q->done.load(std::memory_order_acquire)) return false;
        return true;
    };
    auto take_lead = [&]() -> bool {  // the role may have been handed to any of this call's requests
        bool l = false;
        for (CoReq *q : rs) l = q->lead.exchange(false, std::memory_order_acq_rel) || l;
        return l;
    };
    {
        std::unique_lock<std::mutex> lk(c.mu, std::defer_lock);
        for (;;) {
            if (c.depth.load(std::memory_order_relaxed) > 0) {
                const int rc = co_defer(ctx, rs);
                if (rc >= 0) return rc;  // (-1: deferred mode was switched off while this call waited: it goes the blocking way)
                if (rc == -2) {          // no record for this thread: its launches go out directly, one request at a time
                    Scope sc(&ctx);
                    for (CoReq *q : rs) {
                        ctx.arena_reset();
                        TRY(q->run(q->ops.data(), q->nb));
                    }
                    return HE_OK;
                }
            }
            lk.lock();
            while (c.stop) {  // a dispatcher that is being stopped still launches what it holds: stay out of its way
                const uint32_t g = c.gen.load(std::memory_order_acquire);
                lk.unlock();
                co_sleep(c, g);
                lk.lock();
            }
            if (c.depth.load(std::memory_order_relaxed) <= 0) break;
            lk.unlock();  // (deferred mode was switched on meanwhile)
        }
        const auto now = std::chrono::steady_clock::now();
        const uint64_t me = co_me();
        for (CoReq *q : rs) { q->arrived = now; q->caller = me; q->seq = g_my_calls; c.pending.push_back(q); }
        g_my_calls++;
        co_note_caller(c, me, now);
        bool lead = false;
        if (!c.leader) { c.leader = true; lead = true; }
        else c.cv_leader.notify_one();  // a gathering leader counts arrivals
        for (;;) {
            if (lead) {
                co_lead(ctx, c, lk, r, rs.size() > 1 ? &rs : nullptr);
                // hand the role to the oldest request still waiting (its owner sleeps on the generation word), if any
                if (!c.pending.empty()) { c.pending.front()->lead.store(true, std::memory_order_release); lk.unlock(); co_wake_all(c); }
                else { c.leader = false; lk.unlock(); }
                break;
            }
            lk.unlock();
            // wait for a batch to finish or for the role: read the generation first, then the flags (a bump in between makes the
            // futex wait return at once)
            for (;;) {
                const uint32_t g = c.gen.load(std::memory_order_acquire);
                if (all_done()) break;
                if (take_lead()) { lead = true; break; }
                syscall(SYS_futex, reinterpret_cast<uint32_t *>(&c.gen), FUTEX_WAIT_PRIVATE, g, nullptr, nullptr, 0);
            }
            if (!lead) break;
            lk.lock();
        }
    }
    for (CoReq *q : rs)
        if (q->rc != HE_OK) return fail(q->rc, "%s", q->err.c_str());
    return HE_OK;
}
int co_submit(Ctx &ctx, CoReq &r) { return co_submit_many(ctx, std::vector<CoReq *>{&r}); }
// Every entry point of the one-ciphertext interface ends here: a call over one batch entry on a context whose queue is on (and
// that is not recording a graph: a captured sequence must be this thread's own launches) joins the queue; everything else runs
// its launches at once under the context's lock.
int co_dispatch(Ctx &ctx, int B, CoReq &r) {
    // (handles of a few entries join the queue like single ciphertexts: the drivers stack independent ciphertexts -- the real and
    // imaginary halves of a bootstrap's EvalMod -- into one handle; a request of nb entries takes nb rows of the entry table)
    if (B >= 1 && B < ctx.co->max_batch.load(std::memory_order_relaxed) && !ctx.capturing) {
        r.nb = B;
        r.set_alias_pattern();
        return co_submit(ctx, r);
    }
    Scope sc(&ctx);
    return r.run(r.ops.data(), B);
}

LimbTab ident_tab(int n, int in0 = 0, int out0 = 0, int mod0 = 0) {
    LimbTab t;
    t.n = n;
    for (int i = 0; i < n; i++) {
        t.in_limb[i] = (uint8_t)(in0 + i);
        t.out_limb[i] = (uint8_t)(out0 + i);
        t.mod[i] = (uint8_t)(mod0 + i);
    }
    return t;
}

int check_level(const Ring &r, int level, const char *who) {
    if (level < 0 || level >= r.nmod()) return fail(HE_EINVAL, "%s: level %d out of range [0,%d]", who, level, r.nmod() - 1);
    return HE_OK;
}

// Operand identity (hering.h, Conventions, "aliasing"): one operand of a call, its role and its side.  `p` may be null (an absent
// operand, or one that is no polynomial).  P-side operands are the special-prime parts (limbs of ringP); everything else is Q-side.
struct AliasOp {
    const Poly *p;
    bool out;    // written by the call (outputs and accumulating outputs)
    bool P;      // a P-side operand
    bool bcast;  // an input that may have batch 1 against the call's batch
};
// Checked on the host before anything is filed (also in deferred mode, so the call itself returns the rejection): two operands
// that are the same polynomial are allowed when both are only read, or when they are an (output, input) pair listed in `allowed`
// (indices into `ops`: the in-place forms the reference computes; all_inplace: every such pair).  Two outputs, a Q-side and a
// P-side operand of which one is written, and every other (output, input) pair fail with HE_EINVAL.
int reject_aliasing(const char *who, const AliasOp *ops, size_t n, const std::pair<int, int> *allowed, int n_allowed, bool all_inplace) {
    for (size_t i = 0; i < n; i++) {
        if (!ops[i].p) continue;
        for (size_t j = i + 1; j < n; j++) {
            if (!ops[j].p || ops[i].p->d != ops[j].p->d) continue;
            const AliasOp &a = ops[i], &b = ops[j];
            if (!a.out && !b.out) continue;
            if (a.P != b.P) return fail(HE_EINVAL, "%s: operands %zu and %zu are the same polynomial on the Q and the P side", who, i, j);
            if (a.out && b.out) return fail(HE_EINVAL, "%s: outputs %zu and %zu are the same polynomial", who, i, j);
            bool ok = all_inplace;
            for (int a = 0; a < n_allowed; a++) {
                const auto &pr = allowed[a];
                ok = ok || (pr.first == (int)i && pr.second == (int)j) || (pr.first == (int)j && pr.second == (int)i);
            }
            if (!ok) return fail(HE_EINVAL, "%s: output %zu aliases input %zu (not an in-place form of this operation)", who, a.out ? i : j, a.out ? j : i);
        }
    }
    return HE_OK;
}
// The polynomial operands of one call, each declared ONCE, in the order the request's `run` closure sees them (v[0], v[1], ...).
// in / out / inP / outP check the operand (owner context, degree, limbs, batch), append its view to q.ops and the polynomial to
// q.keep, and return its index -- the name in-place forms (inplace) and identity questions (same) are put with.  A null pointer
// (or opt() of handle 0) is an absent operand: a null view.  The first failure sticks; check() returns it, or else holds the
// broadcast operands against the call's batch and applies the aliasing rule.  Nothing is filed before check() said HE_OK.
struct Operands {
    static constexpr int kCall = -1, kBroadcast = -2;  // batch rules (a value >= 0: exactly that batch)
    CoReq &q;
    const char *who;
    const std::shared_ptr<Ctx> &ctx;  // the owner every operand must share
    const int N;                      // the degree of an operand that names no other
    int B;                            // the call's batch: given, or that of the first operand held to it
    int rc = HE_OK;
    bool all_inplace = false;         // every output may be every input of its side
    bool writes = false;              // some operand is written (only then can identity matter)
    AliasOp few[12], *ops = few;      // the operands declared so far (the lintrans terms and the pack steps spill to `many`)
    std::vector<AliasOp> many;
    int n = 0;
    std::pair<int, int> allowed[4];   // the (output, input) pairs declared with inplace() (no entry point has more than two)
    int n_allowed = 0;
    Operands(CoReq &q, const char *who, const std::shared_ptr<Ctx> &ctx, int N, int B = kCall) : q(q), who(who), ctx(ctx), N(N), B(B) {
        q.ops.reserve(8); q.keep.reserve(12);
    }
    Operands(const Operands &) = delete;  // (`ops` may point into the object)
    Operands(CoReq &q, const char *who, const Ring &r, int B = kCall) : Operands(q, who, r.ctx, r.N, B) {}
    Operands(CoReq &q, const char *who, const BasisExtender &be, int B = kCall) : Operands(q, who, be.ctx, be.Q->N, B) {}
    // a handle that must name a polynomial / that may be 0 (absent)
    std::shared_ptr<Poly> poly(he_handle h, bool optional = false) {
        std::shared_ptr<Poly> p = (optional && !h) ? nullptr : get<Poly>(h, T_POLY);
        if (!p && !(optional && !h) && rc == HE_OK) rc = fail(HE_EHANDLE, "%s: bad Poly handle %llu (operand %zu)", who, (unsigned long long)h, (size_t)n);
        return p;
    }
    std::shared_ptr<Poly> opt(he_handle h) { return poly(h, true); }
    int add(const std::shared_ptr<Poly> &p, bool out, bool P, int limbs, const char *name, int batch, int deg) {
        const int i = push({p.get(), out, P, batch == kBroadcast}, p ? p->view() : View{nullptr, 0});
        writes = writes || out;
        if (!p || rc != HE_OK) return i;
        q.keep.push_back(p);
        char idx[24];
        snprintf(idx, sizeof idx, "operand %d", i);
        if (!name) name = idx;
        if (deg == 0) deg = N;
        if (batch == kCall && B == kCall) B = p->batch;
        const int want = batch == kCall ? B : batch;
        if (p->ctx != ctx) rc = fail(HE_EINVAL, "%s: %s belongs to another context", who, name);
        else if (p->N != deg) rc = fail(HE_EINVAL, "%s: %s has degree %d, %d expected", who, name, p->N, deg);
        else if (p->nlimbs < limbs) rc = fail(HE_EINVAL, "%s: %s has %d limbs, %d needed", who, name, p->nlimbs, limbs);
        else if (want >= 0 && p->batch != want) rc = fail(HE_EINVAL, "%s: batch mismatch (%s has %d entries, %d expected)", who, name, p->batch, want);
        return i;
    }
    template <class H> int in(const H &h, int limbs, const char *name = nullptr, int batch = kCall, int deg = 0) { return add(ptr(h), false, false, limbs, name, batch, deg); }
    template <class H> int out(const H &h, int limbs, const char *name = nullptr, int batch = kCall, int deg = 0) { return add(ptr(h), true, false, limbs, name, batch, deg); }
    template <class H> int inP(const H &h, int limbs, const char *name = nullptr, int batch = kCall) { return add(ptr(h), false, true, limbs, name, batch, 0); }
    template <class H> int outP(const H &h, int limbs, const char *name = nullptr) { return add(ptr(h), true, true, limbs, name, kCall, 0); }
    // an operand that is no polynomial (a hoisting buffer): its view, and what keeps it alive
    int raw(View v, std::shared_ptr<Obj> keep) {
        q.keep.push_back(std::move(keep));
        return push({nullptr, false, false, false}, v);
    }
    // the two QP components of a lazy key switch, (c0Q, c0P, c1Q, c1P) -- indices i .. i + 3; without special primes (levelP < 0)
    // the P handles are ignored (pass 0) and their operands absent
    int qp(bool out, he_handle c0Q, he_handle c0P, he_handle c1Q, he_handle c1P, int levelQ, int levelP) {
        const int i = add(poly(c0Q), out, false, levelQ + 1, "c0Q", kCall, 0);
        add(levelP < 0 ? nullptr : poly(c0P), out, true, levelP + 1, "c0P", kCall, 0);
        add(poly(c1Q), out, false, levelQ + 1, "c1Q", kCall, 0);
        add(levelP < 0 ? nullptr : poly(c1P), out, true, levelP + 1, "c1P", kCall, 0);
        return i;
    }
    void inplace(int o, int i) {
        if (n_allowed < 4) allowed[n_allowed++] = {o, i};
        else if (rc == HE_OK) rc = fail(HE_EINVAL, "%s: internal error, too many in-place forms", who);
    }
    bool same(int i, int j) const { return ops[i].p && ops[j].p && ops[i].p->d == ops[j].p->d; }
    int check() {
        for (int i = 0; i < n && rc == HE_OK; i++) {
            if (!ops[i].bcast || !ops[i].p) continue;
            if (ops[i].p->batch == 1) q.ops[i].bstride = 0;  // one polynomial for every entry of the batch
            else if (ops[i].p->batch != B) rc = fail(HE_EINVAL, "%s: batch mismatch (operand %d has %d entries, 1 or %d expected)", who, i, ops[i].p->batch, B);
        }
        TRY(rc);
        return writes ? reject_aliasing(who, ops, (size_t)n, allowed, n_allowed, all_inplace) : HE_OK;
    }

private:
    int push(const AliasOp &a, View v) {
        if (n == 12) many.assign(few, few + 12);
        if (n >= 12) { many.push_back(a); ops = many.data(); }
        else few[n] = a;
        q.ops.push_back(v);
        return n++;
    }
    const std::shared_ptr<Poly> &ptr(const std::shared_ptr<Poly> &p) { return p; }
    std::shared_ptr<Poly> ptr(he_handle h) { return poly(h); }
};
// Galois elements act through g mod NthRoot (2N, 4N on conjugate-invariant rings): the reduced element is what keys batches and
// index caches, so that g and g + k NthRoot share them
inline uint64_t reduce_gal(uint64_t gal, int logN, int type) { return gal & ((2ull << (logN + type)) - 1); }

uint8_t modulus_class(uint64_t q) { return (q >> 47) == 0 ? 2 : ((q >> 58) == 0 ? 1 : 0); }
// plain (non-Montgomery) twiddles as doubles for the moduli the double-precision row kernel handles
int upload_f64_tables(const std::vector<const SubRingHost *> &subs, int N, double **d_f, double **d_i) {
    const size_t n = subs.size();
    bool any = false;
    for (auto *s : subs) any = any || modulus_class(s->mc.q) == 2;
    *d_f = *d_i = nullptr;
    if (!any) return HE_OK;
    std::vector<double> tf(n * (size_t)N, 0.0), ti(n * (size_t)N, 0.0);
    for (size_t i = 0; i < n; i++) {
        const ModConst &m = subs[i]->mc;
        if (modulus_class(m.q) != 2) continue;
        for (int j = 0; j < N; j++) {
            tf[i * (size_t)N + j] = (double)imform(subs[i]->roots_fwd[j], m.q, m.qinv);
            ti[i * (size_t)N + j] = (double)imform(subs[i]->roots_bwd[j], m.q, m.qinv);
        }
    }
    HIP_TRY(hipMalloc((void **)d_f, tf.size() * sizeof(double)));
    HIP_TRY(hipMalloc((void **)d_i, ti.size() * sizeof(double)));
    HIP_TRY(hipMemcpy(*d_f, tf.data(), tf.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(*d_i, ti.data(), ti.size() * sizeof(double), hipMemcpyHostToDevice));
    return HE_OK;
}
int upload_tables(const std::vector<const SubRingHost *> &subs, int N, ModConst **d_mc, uint64_t **d_twf, uint64_t **d_twi) {
    const size_t n = subs.size();
    std::vector<ModConst> mc(n);
    std::vector<uint64_t> twf(n * (size_t)N), twi(n * (size_t)N);
    for (size_t i = 0; i < n; i++) {
        mc[i] = subs[i]->mc;
        std::copy(subs[i]->roots_fwd.begin(), subs[i]->roots_fwd.end(), twf.begin() + i * (size_t)N);
        std::copy(subs[i]->roots_bwd.begin(), subs[i]->roots_bwd.end(), twi.begin() + i * (size_t)N);
    }
    HIP_TRY(hipMalloc((void **)d_mc, n * sizeof(ModConst)));
    HIP_TRY(hipMalloc((void **)d_twf, twf.size() * sizeof(uint64_t)));
    HIP_TRY(hipMalloc((void **)d_twi, twi.size() * sizeof(uint64_t)));
    HIP_TRY(hipMemcpy(*d_mc, mc.data(), n * sizeof(ModConst), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(*d_twf, twf.data(), twf.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(*d_twi, twi.data(), twi.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    return HE_OK;
}

}  // namespace

static int ctx_set_coalescing(const std::shared_ptr<Ctx> &c, int max_batch, int window_us, const char *who);

extern "C" {

const char *he_last_error(void) { return g_err.c_str(); }
const char *he_version(void) { return "libhering 0.1 (gfx950)"; }

// ---------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------
int he_ctx_create(int device_id, he_handle *out) {
    if (!out) return fail(HE_EINVAL, "he_ctx_create: null output");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(HE_EDEVICE, "he_ctx_create: no HIP device available (%s); libhering has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= ndev) return fail(HE_EINVAL, "he_ctx_create: device %d out of range [0,%d)", device_id, ndev);
    auto c = std::make_shared<Ctx>();
    c->dev = device_id;
    HIP_TRY(hipSetDevice(device_id));
    HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&c->ev0));
    HIP_TRY(hipEventCreate(&c->ev1));
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b > 0) c->kPoolCap = std::max<size_t>(c->kPoolCap, total_b / 2);
        else (void)hipGetLastError();
    }
    *out = reg(c);
    // HERING_QUEUE_DEFAULT="max_batch,window_us[,depth]" (soak runs): every context starts with its submission queue on (and, with a
    // depth, in deferred mode) -- the whole test suite then exercises the queued paths with single-threaded callers
    if (const char *qd = getenv("HERING_QUEUE_DEFAULT")) {
        int mb = 0, win = 0, depth = 0;
        const int n = sscanf(qd, "%d,%d,%d", &mb, &win, &depth);
        if (n >= 2 && mb > 1) {
            TRY(ctx_set_coalescing(c, mb, win, "HERING_QUEUE_DEFAULT"));
            if (n >= 3 && depth > 0) TRY(he_ctx_set_deferred(*out, depth));
        }
    }
    return HE_OK;
}
int he_ctx_destroy(he_handle h) {
    {
        GET(c, Ctx, h, T_CTX);
        co_stop_dispatcher(*c);  // (deferred submission: everything pending is launched; objects that outlive the handle call directly)
    }
    return unreg(h, T_CTX);
}
int he_device_count(int *n) {
    if (!n) return fail(HE_EINVAL, "he_device_count: null output");
    *n = 0;
    const hipError_t e = hipGetDeviceCount(n);
    if (e != hipSuccess) { (void)hipGetLastError(); *n = 0; }  // no driver / no device: zero, not an error
    return HE_OK;
}
int he_debug_device_pci_bus_id(int device, char *out, int len) {
    if (!out || len < 13) return fail(HE_EINVAL, "he_debug_device_pci_bus_id: buffer of at least 13 bytes");
    out[0] = 0;
    if (hipDeviceGetPCIBusId(out, len, device) != hipSuccess) { (void)hipGetLastError(); out[0] = 0; return fail(HE_EDEVICE, "he_debug_device_pci_bus_id: no such device"); }
    return HE_OK;
}
int he_ctx_sync(he_handle h) {
    GET(c, Ctx, h, T_CTX);
    if (c->capturing) return fail(HE_EINVAL, "he_ctx_sync: the context is capturing a graph (he_graph_end first)");
    // deferred submission: everything filed before this call is launched first; a launch that failed after its call had returned
    // is reported here -- AFTER the stream has been drained (the caller that is told about a failure must not find the
    // device still running the requests that preceded it)
    int filed_rc = HE_OK;
    std::string filed_msg;
    if (c->co->depth.load(std::memory_order_relaxed) > 0 && (filed_rc = co_flush_filed(*c)) != HE_OK) filed_msg = he_last_error();
    // Many threads may wait on one context at once (the callers of a coalescing evaluator): ONE of them drains the stream, the
    // others sleep until a drain that STARTED after their call began has finished -- everything a caller enqueued before calling
    // is covered by such a drain -- instead of every thread spinning on the stream.
    std::unique_lock<std::mutex> lk(c->sync_mu);
    const uint64_t ticket = ++c->sync_tickets;
    struct Waiting { int &n; explicit Waiting(int &x) : n(x) { n++; } ~Waiting() { n--; } } waiting(c->sync_waiters);
    while (c->sync_covered < ticket) {
        if (c->syncing && c->sync_waiters > 8) { c->sync_cv.wait(lk); continue; }  // a crowd sleeps: its spinning would eat the CPUs the callers need
        if (c->syncing) {
            // a short drain is cheaper to wait out on the CPU than through a futex sleep and its wake-up latency (a handful of
            // callers waiting for a small batch); a long one (dozens of callers, a batch of a millisecond) is slept through
            const auto t0 = std::chrono::steady_clock::now();
            bool covered = false;
            while (std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(150)) {
                lk.unlock();
                sched_yield();
                lk.lock();
                if (c->sync_covered >= ticket || !c->syncing) { covered = true; break; }
            }
            if (!covered) c->sync_cv.wait(lk);
            continue;
        }
        c->syncing = true;
        const uint64_t covers = c->sync_tickets;
        lk.unlock();
        hipError_t e = hipSetDevice(c->dev);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        lk.lock();
        c->syncing = false;
        if (e == hipSuccess) c->sync_covered = std::max(c->sync_covered, covers);
        c->sync_cv.notify_all();
        if (e != hipSuccess) return fail(HE_EDEVICE, "he_ctx_sync: %s", hipGetErrorString(e));
    }
    if (filed_rc != HE_OK) return fail(filed_rc, "%s", filed_msg.c_str());
    return HE_OK;
}
int he_timer_start(he_handle h) {
    GET(c, Ctx, h, T_CTX);
    if (c->co->depth.load(std::memory_order_relaxed) > 0) TRY(co_flush_filed(*c));  // (the timed region covers what was filed)
    HIP_TRY(hipSetDevice(c->dev));
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    return HE_OK;
}
int he_timer_stop(he_handle h, float *ms) {
    GET(c, Ctx, h, T_CTX);
    if (c->co->depth.load(std::memory_order_relaxed) > 0) TRY(co_flush_filed(*c));  // (the timed region covers what was filed)
    HIP_TRY(hipSetDevice(c->dev));
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    HIP_TRY(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return HE_OK;
}
int he_device_info(he_handle h, uint64_t out[4]) {
    GET(c, Ctx, h, T_CTX);
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, c->dev));
    out[0] = (uint64_t)p.multiProcessorCount;
    out[1] = (uint64_t)p.maxSharedMemoryPerMultiProcessor;
    out[2] = (uint64_t)p.clockRate;
    out[3] = (uint64_t)p.totalGlobalMem;
    return HE_OK;
}

// ---------------------------------------------------------------------------------------
// ring
// ---------------------------------------------------------------------------------------
int he_ring_create(he_handle hctx, int logN, const uint64_t *moduli, int n, he_handle *out) {
    return he_ring_create_type(hctx, logN, 0, moduli, n, out);
}
int he_ring_create_type(he_handle hctx, int logN, int ring_type, const uint64_t *moduli, int n, he_handle *out) {
    GET(c, Ctx, hctx, T_CTX);
    if (ring_type != 0 && ring_type != 1) return fail(HE_EINVAL, "he_ring_create: invalid ring type %d", ring_type);
    if (!moduli || !out || n <= 0) return fail(HE_EINVAL, "he_ring_create: invalid ModuliChain (must be a non-empty []uint64)");
    if (n > 48) return fail(HE_EINVAL, "he_ring_create: at most 48 moduli per ring");
    if (logN < 4 || logN > kMaxLogN) return fail(HE_EPARAM, "he_ring_create: logN=%d outside [4,%d]", logN, kMaxLogN);
    for (int i = 0; i < n; i++)
        for (int j = i + 1; j < n; j++)
            if (moduli[i] == moduli[j]) return fail(HE_EPARAM, "he_ring_create: invalid ModuliChain (moduli are not distinct)");
    auto r = std::make_shared<Ring>();
    r->ctx = c;
    r->logN = logN;
    r->N = 1 << logN;
    r->moduli.assign(moduli, moduli + n);
    r->sub.resize(n);
    r->type = ring_type;
    std::string err;
    for (int i = 0; i < n; i++)
        if (!(ring_type ? build_subring_ci(logN, moduli[i], r->sub[i], err) : build_subring(logN, moduli[i], r->sub[i], err)))
            return fail(HE_EPARAM, "he_ring_create: %s", err.c_str());
    r->rescale = build_rescale_constants(r->moduli);
    Scope sc(c.get());
    std::vector<const SubRingHost *> subs;
    for (auto &s : r->sub) subs.push_back(&s);
    TRY(upload_tables(subs, r->N, &r->d_mc, &r->d_twf, &r->d_twi));
    for (uint64_t m : r->moduli) r->small.push_back(modulus_class(m));
    TRY(upload_f64_tables(subs, r->N, &r->d_twdf, &r->d_twdi));
    r->dev = RingDev{logN, r->N, r->d_mc, r->d_twf, r->d_twi, r->small.data(), r->d_twdf, r->d_twdi};
    *out = reg(r);
    return HE_OK;
}
int he_ring_destroy(he_handle h) { return unreg(h, T_RING); }
int he_ring_constant(he_handle h, int limb, int which, uint64_t *out) {
    GET(r, Ring, h, T_RING);
    if (limb < 0 || limb >= r->nmod() || !out) return fail(HE_EINVAL, "he_ring_constant: bad limb");
    const SubRingHost &s = r->sub[limb];
    switch (which) {
        case 0: *out = s.mc.q; break;
        case 1: *out = s.mc.qinv; break;
        case 2: *out = s.mc.brc0; break;
        case 3: *out = s.mc.brc1; break;
        case 4: *out = s.mc.ninv; break;
        case 5: *out = s.primroot; break;
        default: return fail(HE_EINVAL, "he_ring_constant: bad selector %d", which);
    }
    return HE_OK;
}
int he_ring_roots(he_handle h, int limb, int dir, uint64_t *out) {
    GET(r, Ring, h, T_RING);
    if (limb < 0 || limb >= r->nmod() || !out) return fail(HE_EINVAL, "he_ring_roots: bad limb");
    Scope sc(r->ctx.get());
    HIP_TRY(hipStreamSynchronize(r->ctx->stream));
    HIP_TRY(hipMemcpy(out, (dir ? r->d_twi : r->d_twf) + (size_t)limb * r->N, (size_t)r->N * 8, hipMemcpyDeviceToHost));
    return HE_OK;
}

// ---------------------------------------------------------------------------------------
// polynomials
// ---------------------------------------------------------------------------------------
static int poly_alloc(he_handle hring, int n_limbs, int batch, bool zero, he_handle *out) {
    GET(r, Ring, hring, T_RING);
    if (n_limbs <= 0 || n_limbs > 255 || batch <= 0 || !out) return fail(HE_EINVAL, "he_poly_alloc: bad shape (%d limbs, batch %d)", n_limbs, batch);
    auto p = std::make_shared<Poly>();
    p->ctx = r->ctx;
    p->N = r->N;
    p->nlimbs = n_limbs;
    p->batch = batch;
    const size_t bytes = (size_t)batch * n_limbs * r->N * 8;
    // scratch polynomials: contents unspecified (a recycled buffer); HERING_POISON=1 fills them with a pattern so that a
    // read-before-write shows up as a parity failure instead of depending on what the buffer held
    static const bool poison = env_flag("HERING_POISON");
    // (the buffer cache has its own lock: only a fill is stream work that needs the context -- a scratch allocation of one caller
    // does not wait for the launches of another's batch)
    HIP_TRY(hipSetDevice(r->ctx->dev));
    hipError_t e = r->ctx->pool_take(bytes, (void **)&p->d);
    if (e != hipSuccess) {
        p->d = nullptr;
        return fail(HE_ENOMEM, "he_poly_alloc: hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    }
    Ctx &cx = *r->ctx;
    // Deferred submission: the fill must be ON THE STREAM when this call returns -- a handle may be handed to another thread (or a
    // goroutine may migrate between NewPoly and Upload), and a direct launch of that thread (upload, batched call) only waits for
    // ITS OWN pending requests: a fill still sitting in the allocating thread's queue would land on top of the other thread's data
    // (ADVICE r5).  So with a dispatcher the fill is a stream-ordered memset right here (NoFlush: a buffer fresh from the cache is
    // addressed by no pending request); measured equal on the c5 replay (85.4 bootstraps/s either way, NOTES.md round 5).
    const bool deferred = cx.co->depth.load(std::memory_order_relaxed) > 0;
    if (zero && !poison && !deferred && n_limbs <= kMaxLimbs && batch < cx.co->max_batch.load(std::memory_order_relaxed) && !cx.capturing) {
        // queue on (default mode: a call returns once its batch is enqueued): the zero fills of concurrent callers' fresh polynomials
        // are one launch over an entry table like any other request (16 callers replaying a bootstrap issued 44 memsets each per
        // bootstrap, every one under the context's lock)
        const std::shared_ptr<Ctx> ctx = r->ctx;
        const int N = r->N;
        CoReq q;
        q.op = CO_ZERO; q.obj = ctx.get(); q.par[0] = n_limbs; q.par[1] = N;
        q.ops = {p->view()};
        q.keep = {p};
        q.run = [ctx, n_limbs, N](const View *v, int B) -> int {
            if (!v[0].tab) {  // one request: its entries are contiguous
                HIP_TRY(hipMemsetAsync(v[0].p, 0, (size_t)B * n_limbs * N * 8, ctx->stream));
                return HE_OK;
            }
            RingDev dev{};
            dev.N = N;
            HIP_TRY(launch_ew(dev, ident_tab(n_limbs), EW_ZERO, v[0], v[0], v[0], B, nullptr, nullptr, ctx->stream));
            return HE_OK;
        };
        TRY(co_dispatch(cx, batch, q));
    } else if (zero || poison) {
        Scope sc(r->ctx.get(), NoFlush{});  // (no pending request can address a buffer that was in the cache)
        HIP_TRY(hipMemsetAsync(p->d, zero ? 0 : 0x5a, bytes, r->ctx->stream));
    }
    *out = reg(p);
    return HE_OK;
}
int he_poly_alloc(he_handle hring, int n_limbs, int batch, he_handle *out) { return poly_alloc(hring, n_limbs, batch, true, out); }
int he_poly_alloc_scratch(he_handle hring, int n_limbs, int batch, he_handle *out) { return poly_alloc(hring, n_limbs, batch, false, out); }
int he_poly_free(he_handle h) { return unreg(h, T_POLY); }
int he_poly_shape(he_handle h, int *n_limbs, int *batch, int *N) {
    GET(p, Poly, h, T_POLY);
    if (n_limbs) *n_limbs = p->nlimbs;
    if (batch) *batch = p->batch;
    if (N) *N = p->N;
    return HE_OK;
}
int he_poly_upload(he_handle h, const uint64_t *src, size_t n_words) {
    GET(p, Poly, h, T_POLY);
    const size_t total = (size_t)p->batch * p->nlimbs * p->N;
    if (!src || n_words != total) return fail(HE_EINVAL, "he_poly_upload: expected %zu words, got %zu", total, n_words);
    if (p->ctx->capturing) return fail(HE_EINVAL, "he_poly_upload: host transfers cannot be captured in a graph");
    Scope sc(p->ctx.get());
    HIP_TRY(hipMemcpyAsync(p->d, src, total * 8, hipMemcpyHostToDevice, p->ctx->stream));
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    return HE_OK;
}
int he_poly_download(he_handle h, uint64_t *dst, size_t n_words) {
    GET(p, Poly, h, T_POLY);
    const size_t total = (size_t)p->batch * p->nlimbs * p->N;
    if (!dst || n_words != total) return fail(HE_EINVAL, "he_poly_download: expected %zu words, got %zu", total, n_words);
    if (p->ctx->capturing) return fail(HE_EINVAL, "he_poly_download: host transfers cannot be captured in a graph");
    Scope sc(p->ctx.get());
    HIP_TRY(hipMemcpyAsync(dst, p->d, total * 8, hipMemcpyDeviceToHost, p->ctx->stream));
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    return HE_OK;
}
int he_poly_upload_limb(he_handle h, int b, int limb, const uint64_t *src) {
    GET(p, Poly, h, T_POLY);
    if (!src || b < 0 || b >= p->batch || limb < 0 || limb >= p->nlimbs) return fail(HE_EINVAL, "he_poly_upload_limb: bad index");
    if (p->ctx->capturing) return fail(HE_EINVAL, "he_poly_upload_limb: host transfers cannot be captured in a graph");
    Scope sc(p->ctx.get());
    HIP_TRY(hipMemcpyAsync(p->d + ((size_t)b * p->nlimbs + limb) * p->N, src, (size_t)p->N * 8, hipMemcpyHostToDevice, p->ctx->stream));
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    return HE_OK;
}
int he_poly_download_limb(he_handle h, int b, int limb, uint64_t *dst) {
    GET(p, Poly, h, T_POLY);
    if (!dst || b < 0 || b >= p->batch || limb < 0 || limb >= p->nlimbs) return fail(HE_EINVAL, "he_poly_download_limb: bad index");
    if (p->ctx->capturing) return fail(HE_EINVAL, "he_poly_download_limb: host transfers cannot be captured in a graph");
    Scope sc(p->ctx.get());
    HIP_TRY(hipMemcpyAsync(dst, p->d + ((size_t)b * p->nlimbs + limb) * p->N, (size_t)p->N * 8, hipMemcpyDeviceToHost, p->ctx->stream));
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));
    return HE_OK;
}
// the request of a copy of limbs 0..level, v[0] -> v[1]: a device-to-device memcpy, or one EW_COPY launch over an entry table
static void copy_request(CoReq &q, const std::shared_ptr<Ctx> &ctx, int level, int N) {
    q.op = CO_COPY; q.obj = ctx.get(); q.par[0] = level; q.par[1] = N;
    q.run = [ctx, level, N](const View *v, int B) -> int {
        ctx->acct(2.0 * (level + 1), 0, B, N);
        if (!v[0].tab && !v[1].tab) {
            HIP_TRY(hipMemcpy2DAsync(v[1].p, v[1].bstride * 8, v[0].p, v[0].bstride * 8, (size_t)(level + 1) * N * 8, B, hipMemcpyDeviceToDevice,
                                     ctx->stream));
            return HE_OK;
        }
        RingDev dev{};  // EW_COPY reads no modulus record and no table: degree and strides are all it needs
        dev.N = N;
        HIP_TRY(launch_ew(dev, ident_tab(level + 1), EW_COPY, v[0], v[0], v[1], B, nullptr, nullptr, ctx->stream));
        return HE_OK;
    };
}
int he_poly_copy(he_handle hdst, he_handle hsrc, int level) {
    GET(d, Poly, hdst, T_POLY);
    GET(s, Poly, hsrc, T_POLY);
    if (level < 0) return fail(HE_EINVAL, "he_poly_copy: negative level");
    const std::shared_ptr<Ctx> ctx = d->ctx;
    const int N = d->N;
    CoReq q;
    Operands o(q, "he_poly_copy", ctx, N);
    const int is = o.in(s, level + 1, "src"), id = o.out(d, level + 1, "dst");
    o.inplace(id, is);
    TRY(o.check());
    if (o.same(is, id)) return HE_OK;  // Poly.CopyLvl onto itself: nothing to copy (and no overlapping memcpy to file)
    // (the copies of concurrent single-ciphertext callers ride in the queue like every other operation: one EW_COPY launch over an
    // entry table; a lone copy is a device-to-device memcpy as before)
    copy_request(q, ctx, level, N);
    return co_dispatch(*ctx, d->batch, q);
}
int he_poly_copy_batch(he_handle hdst, int dst_b0, he_handle hsrc, int src_b0, int nb, int level) {
    GET(d, Poly, hdst, T_POLY);
    GET(s, Poly, hsrc, T_POLY);
    if (d->N != s->N || level < 0 || d->nlimbs < level + 1 || s->nlimbs < level + 1 || nb <= 0 || dst_b0 < 0 || src_b0 < 0 ||
        dst_b0 + nb > d->batch || src_b0 + nb > s->batch || d->ctx != s->ctx)
        return fail(HE_EINVAL, "he_poly_copy_batch: shape mismatch");
    // overlapping entry ranges of one handle are rejected (hering.h): the copy launches give no order between entries
    if (d->d == s->d && dst_b0 < src_b0 + nb && src_b0 < dst_b0 + nb)
        return fail(HE_EINVAL, "he_poly_copy_batch: the entry ranges [%d,%d) and [%d,%d) of one polynomial overlap", src_b0, src_b0 + nb, dst_b0,
                    dst_b0 + nb);
    // (a copy between entry ranges of two handles: the request of he_poly_copy over shifted views)
    const std::shared_ptr<Ctx> ctx = d->ctx;
    const int N = d->N;
    CoReq q;
    View vs = s->view(), vd = d->view();
    vs.p += (size_t)src_b0 * vs.bstride; vd.p += (size_t)dst_b0 * vd.bstride;
    q.ops = {vs, vd};  // (entry ranges, possibly of one handle: the overlap rule above is this call's own -- not an Operands list)
    q.keep = {s, d};
    copy_request(q, ctx, level, N);
    return co_dispatch(*ctx, nb, q);
}
int he_poly_device_buffer(he_handle h, void **ptr, size_t *bytes) {
    GET(p, Poly, h, T_POLY);
    if (!ptr || !bytes) return fail(HE_EINVAL, "he_poly_device_buffer: null output");
    Scope sc(p->ctx.get());
    HIP_TRY(hipStreamSynchronize(p->ctx->stream));  // the caller reads / writes it on a stream of its own
    *ptr = p->d;
    *bytes = (size_t)p->batch * p->nlimbs * p->N * 8;
    return HE_OK;
}
int he_poly_zero(he_handle h) {
    GET(p, Poly, h, T_POLY);
    Scope sc(p->ctx.get());
    HIP_TRY(hipMemsetAsync(p->d, 0, (size_t)p->batch * p->nlimbs * p->N * 8, p->ctx->stream));
    return HE_OK;
}

// ---------------------------------------------------------------------------------------
// NTT (ring/ntt.go:127-152)
// ---------------------------------------------------------------------------------------
// NTT of a Ring of either type: the conjugate-invariant transform is a fold around the standard
// network (ring/ntt.go:716-1311)
static hipError_t typed_ntt(const RingDev &dev, int type, hipStream_t st, const LimbTab &tab, View in, View out, int batch,
                            bool inverse, int flags) {
    if (type == 0) return launch_ntt(dev, tab, in, out, batch, inverse, flags, st);
    LimbTab oo = tab;  // second step works in place on `out`
    for (int i = 0; i < tab.n; i++) oo.in_limb[i] = tab.out_limb[i];
    hipError_t e;
    if (!inverse) {
        if ((e = launch_ci_fold(dev, tab, in, out, batch, false, (flags & NTT_REDUCE_INPUT) != 0, st)) != hipSuccess) return e;
        return launch_ntt(dev, oo, out, out, batch, false, flags & ~NTT_REDUCE_INPUT, st);
    }
    if ((e = launch_ntt(dev, tab, in, out, batch, true, flags, st)) != hipSuccess) return e;
    return launch_ci_fold(dev, oo, out, out, batch, true, false, st);
}
static hipError_t ring_ntt(const Ring &r, const LimbTab &tab, View in, View out, int batch, bool inverse, int flags) {
    return typed_ntt(r.dev, r.type, r.ctx->stream, tab, in, out, batch, inverse, flags);
}

// NTT over the combined QP table of a basis extender / evaluator, of either ring type
static hipError_t be_ntt(const BasisExtender &be, const LimbTab &tab, View in, View out, int batch, bool inverse, int flags) {
    return typed_ntt(be.qp, be.type, be.ctx->stream, tab, in, out, batch, inverse, flags);
}

// the operands of the ring's one-input operations, each computed in place by the reference: p1 -> p2 at `level`
// (B: the call's batch; inplace: whether p1 and p2 are one polynomial)
static int unary_operands(CoReq &q, const char *who, const std::shared_ptr<Ring> &r, int level, he_handle h1, he_handle h2, int *B,
                          bool *inplace = nullptr) {
    TRY(check_level(*r, level, who));
    Operands o(q, who, *r);
    o.in(h1, level + 1);
    o.out(h2, level + 1);
    o.all_inplace = true;
    q.keep.push_back(r);
    TRY(o.check());
    *B = o.B;
    if (inplace) *inplace = o.same(0, 1);
    return HE_OK;
}
static int ntt_api(he_handle hring, int level, he_handle h1, he_handle h2, bool inverse, int flags, const char *who) {
    GET(r, Ring, hring, T_RING);
    CoReq q;
    int B = 0;
    TRY(unary_operands(q, who, r, level, h1, h2, &B));
    q.op = CO_NTT; q.obj = r.get(); q.par[0] = level; q.par[1] = inverse; q.par[2] = flags;
    q.run = [r, level, inverse, flags](const View *v, int B) -> int {
        r->ctx->acct(2.0 * (level + 1), 0, B, r->N);  // NTT / INTT: 2 L limbs
        { Valu V(r->logN); for (int i = 0; i <= level; i++) V.ntt(cls_f64(r->small, i)); V.into(*r->ctx, B); }
        HIP_TRY(ring_ntt(*r, ident_tab(level + 1), v[0], v[1], B, inverse, flags | NTT_REDUCE_INPUT));
        return HE_OK;
    };
    q.tables_ok = [r](bool *ok) -> int { *ok = r->type == 0; return HE_OK; };  // (the conjugate-invariant fold takes no entry tables)
    return co_dispatch(*r->ctx, B, q);
}
int he_ntt(he_handle r, int level, he_handle p1, he_handle p2) { return ntt_api(r, level, p1, p2, false, 0, "he_ntt"); }
int he_ntt_lazy(he_handle r, int level, he_handle p1, he_handle p2) { return ntt_api(r, level, p1, p2, false, NTT_LAZY_OUT, "he_ntt_lazy"); }
int he_intt(he_handle r, int level, he_handle p1, he_handle p2) { return ntt_api(r, level, p1, p2, true, 0, "he_intt"); }
int he_intt_lazy(he_handle r, int level, he_handle p1, he_handle p2) { return ntt_api(r, level, p1, p2, true, 0, "he_intt_lazy"); }

int he_subring_ntt_host(he_handle hring, int limb, int backward, int lazy, const uint64_t *p1, uint64_t *p2) {
    GET(r, Ring, hring, T_RING);
    if (!p1 || !p2 || limb < 0 || limb >= r->nmod()) return fail(HE_EINVAL, "he_subring_ntt_host: bad arguments");
    Scope sc(r->ctx.get());
    const size_t N = r->N;
    TRY(r->ctx->arena_reserve(N));
    uint64_t *buf = r->ctx->arena_take(N);
    hipStream_t st = r->ctx->stream;
    HIP_TRY(hipMemcpyAsync(buf, p1, N * 8, hipMemcpyHostToDevice, st));
    LimbTab t; t.n = 1; t.in_limb[0] = 0; t.out_limb[0] = 0; t.mod[0] = (uint8_t)limb;
    View v{buf, N};
    HIP_TRY(ring_ntt(*r, t, v, v, 1, backward != 0, NTT_REDUCE_INPUT | ((lazy && !backward) ? NTT_LAZY_OUT : 0)));
    HIP_TRY(hipMemcpyAsync(p2, buf, N * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return HE_OK;
}

// ---------------------------------------------------------------------------------------
// coefficient-wise ops (ring/operations.go)
// ---------------------------------------------------------------------------------------
int he_binop(he_handle hring, int level, int op, he_handle h1, he_handle h2, he_handle h3) {
    GET(r, Ring, hring, T_RING);
    if (op < 0 || op >= HE_BINOP_COUNT) return fail(HE_EINVAL, "he_binop: unknown op %d", op);
    TRY(check_level(*r, level, "he_binop"));
    CoReq q;
    Operands o(q, "he_binop", *r);
    // an input of batch 1 broadcasts over the batch of the output (one plaintext against a batch of ciphertexts)
    o.in(h1, level + 1, nullptr, Operands::kBroadcast);
    o.in(h2, level + 1, nullptr, Operands::kBroadcast);
    o.out(h3, level + 1);
    o.all_inplace = true;
    TRY(o.check());
    q.op = CO_EW; q.obj = r.get(); q.par[0] = level; q.par[1] = op;
    q.keep.push_back(r);
    q.run = [r, level, op](const View *v, int B) -> int {
        // binary 3 L, ...ThenAdd / ...ThenSub 4 L; a batch-1 operand is read once for the whole batch
        const bool then = op == EW_MUL_BARRETT_THEN_ADD || op == EW_MUL_BARRETT_THEN_ADD_LAZY || (op >= EW_MUL_MONT_THEN_ADD && op <= EW_MUL_MONT_LAZY_THEN_SUB_LAZY);
        const double sh = (double)(v[0].bstride == 0 && !v[0].tab && B > 1) + (double)(v[1].bstride == 0 && !v[1].tab && B > 1);
        r->ctx->acct(((then ? 4.0 : 3.0) - sh) * (level + 1), sh * (level + 1), B, r->N);
        if (op >= EW_MUL_BARRETT) { Valu V(r->logN); for (int i = 0; i <= level; i++) V.mul(cls_f64(r->small, i), 1.0); V.into(*r->ctx, B); }
        HIP_TRY(launch_ew(r->dev, ident_tab(level + 1), op, v[0], v[1], v[2], B, nullptr, nullptr, r->ctx->stream));
        return HE_OK;
    };
    return co_dispatch(*r->ctx, o.B, q);
}
int he_unop(he_handle hring, int level, int op, he_handle h1, he_handle h2) {
    GET(r, Ring, hring, T_RING);
    if (op < 0 || op >= HE_UNOP_COUNT) return fail(HE_EINVAL, "he_unop: unknown op %d", op);
    CoReq q;
    int B = 0;
    TRY(unary_operands(q, "he_unop", r, level, h1, h2, &B));
    q.op = CO_EW; q.obj = r.get(); q.par[0] = level; q.par[1] = EW_NEG + op;
    q.run = [r, level, op](const View *v, int B) -> int {
        r->ctx->acct(2.0 * (level + 1), 0, B, r->N);  // unary: 2 L
        if (EW_NEG + op >= EW_MFORM && EW_NEG + op <= EW_IMFORM) { Valu V(r->logN); for (int i = 0; i <= level; i++) V.mul(cls_f64(r->small, i), 1.0); V.into(*r->ctx, B); }
        HIP_TRY(launch_ew(r->dev, ident_tab(level + 1), EW_NEG + op, v[0], v[0], v[1], B, nullptr, nullptr, r->ctx->stream));
        return HE_OK;
    };
    return co_dispatch(*r->ctx, B, q);
}
// scalar given per limb (already what the kernel consumes)
static int scalar_launch(const std::shared_ptr<Ring> &r, int level, int ewop, he_handle h1, he_handle h2, const ScalarTab &st,
                         const char *who, bool dbl = false) {
    CoReq q;
    int B = 0;
    TRY(unary_operands(q, who, r, level, h1, h2, &B));
    q.op = dbl ? CO_EW_DOUBLE : CO_EW; q.obj = r.get(); q.par[0] = level; q.par[1] = ewop; q.par[2] = 1;  // (par[2]: a scalar form)
    q.blob.assign(st.s, st.s + level + 1);
    if (dbl) q.blob.insert(q.blob.end(), st.s2, st.s2 + level + 1);
    q.run = [r, level, ewop, st, dbl](const View *v, int B) -> int {
        r->ctx->acct((ewop == EW_MUL_SCALAR_MONT_THEN_ADD ? 3.0 : 2.0) * (level + 1), 0, B, r->N);  // unary (3 L with the addend)
        if (ewop == EW_MUL_SCALAR_MONT || ewop == EW_MUL_SCALAR_MONT_THEN_ADD) { Valu V(r->logN); for (int i = 0; i <= level; i++) V.mul(cls_f64(r->small, i), 1.0); V.into(*r->ctx, B); }
        if (dbl) HIP_TRY(launch_ew_double(r->dev, ident_tab(level + 1), ewop, v[0], v[1], B, &st, r->ctx->stream));
        else HIP_TRY(launch_ew(r->dev, ident_tab(level + 1), ewop, v[0], v[0], v[1], B, &st, nullptr, r->ctx->stream));
        return HE_OK;
    };
    return co_dispatch(*r->ctx, B, q);
}
int he_scalarop(he_handle hring, int level, int op, he_handle h1, uint64_t scalar, he_handle h2) {
    GET(r, Ring, hring, T_RING);
    TRY(check_level(*r, level, "he_scalarop"));
    ScalarTab st{};
    int ewop;
    for (int i = 0; i <= level; i++) {
        const ModConst &m = r->sub[i].mc;
        switch (op) {
            case HE_ADD_SCALAR: st.s[i] = scalar; break;                                   // operations.go:151 (no reduction of the scalar)
            case HE_SUB_SCALAR: st.s[i] = scalar; break;                                   // :186
            case HE_MUL_SCALAR:                                                            // :201  MForm(scalar)
            case HE_MUL_SCALAR_THEN_ADD: st.s[i] = mform(scalar, m.q, m.brc0, m.brc1); break;  // :208
            case HE_MUL_SCALAR_THEN_SUB:                                                   // :223  MForm(q - BRedAdd(scalar))
                st.s[i] = mform(m.q - bred_add(scalar, m.q, m.brc0), m.q, m.brc0, m.brc1);
                break;
            default: return fail(HE_EINVAL, "he_scalarop: unknown op %d", op);
        }
    }
    switch (op) {
        case HE_ADD_SCALAR: ewop = EW_ADD_SCALAR; break;
        case HE_SUB_SCALAR: ewop = EW_SUB_SCALAR; break;
        case HE_MUL_SCALAR: ewop = EW_MUL_SCALAR_MONT; break;
        default: ewop = EW_MUL_SCALAR_MONT_THEN_ADD; break;
    }
    return scalar_launch(r, level, ewop, h1, h2, st, "he_scalarop");
}
int he_mul_rns_scalar_montgomery(he_handle hring, int level, he_handle h1, const uint64_t *scalar, he_handle h2) {
    GET(r, Ring, hring, T_RING);
    TRY(check_level(*r, level, "he_mul_rns_scalar_montgomery"));
    if (!scalar) return fail(HE_EINVAL, "he_mul_rns_scalar_montgomery: bad arguments");
    ScalarTab st{};
    for (int i = 0; i <= level; i++) st.s[i] = scalar[i];
    return scalar_launch(r, level, EW_MUL_SCALAR_MONT, h1, h2, st, "he_mul_rns_scalar_montgomery");
}
static int bigint_api(he_handle hring, int level, he_handle h1, const uint64_t *words, int nw, he_handle h2, int kind) {
    GET(r, Ring, hring, T_RING);
    TRY(check_level(*r, level, "he_*_scalar_bigint"));
    if (!words || nw <= 0) return fail(HE_EINVAL, "he_*_scalar_bigint: bad arguments");
    ScalarTab st{};
    for (int i = 0; i <= level; i++) {
        const ModConst &m = r->sub[i].mc;
        const uint64_t v = words_mod(words, nw, m.q);
        st.s[i] = kind >= 2 ? mform(v, m.q, m.brc0, m.brc1) : v;
    }
    return scalar_launch(r, level, kind == 0 ? EW_ADD_SCALAR : (kind == 1 ? EW_SUB_SCALAR : (kind == 2 ? EW_MUL_SCALAR_MONT : EW_MUL_SCALAR_MONT_THEN_ADD)), h1, h2, st, "he_*_scalar_bigint");
}
int he_mul_scalar_bigint_then_add(he_handle r, int l, he_handle p1, const uint64_t *w, int n, he_handle p2) { return bigint_api(r, l, p1, w, n, p2, 3); }
int he_double_rns_scalarop(he_handle hring, int level, int op, he_handle h1, const uint64_t *s0, const uint64_t *s1, he_handle h2) {
    GET(r, Ring, hring, T_RING);
    const char *who = "he_double_rns_scalarop";
    TRY(check_level(*r, level, who));
    if (!s0 || !s1 || op < 0 || op > 3) return fail(HE_EINVAL, "%s: bad arguments", who);
    ScalarTab st{};
    for (int i = 0; i <= level; i++) {
        const ModConst &m = r->sub[i].mc;
        st.s[i] = op >= 2 ? mform(s0[i], m.q, m.brc0, m.brc1) : s0[i];
        st.s2[i] = op >= 2 ? mform(s1[i], m.q, m.brc0, m.brc1) : s1[i];
    }
    static const int ops[4] = {EW_ADD_SCALAR, EW_SUB_SCALAR, EW_MUL_SCALAR_MONT, EW_MUL_SCALAR_MONT_THEN_ADD};
    return scalar_launch(r, level, ops[op], h1, h2, st, who, true);
}
static int shift_api(he_handle hring, int level, he_handle h1, int k, he_handle h2, bool monomial, const char *who) {
    GET(r, Ring, hring, T_RING);
    CoReq q;
    int batch = 0;
    bool inplace = false;
    TRY(unary_operands(q, who, r, level, h1, h2, &batch, &inplace));
    const int N = r->N;
    const int period = monomial ? 2 * N : N;
    int kk = k % period;
    if (kk < 0) kk += period;
    q.op = CO_SHIFT; q.obj = r.get(); q.par[0] = level; q.par[1] = kk; q.par[2] = monomial;
    q.run = [r, level, kk, monomial, inplace, N](const View *v, int B) -> int {
        r->ctx->acct(2.0 * (level + 1), 0, B, N);
        View in = v[0];
        const LimbTab tab = ident_tab(level + 1);
        if (inplace) {  // in place: stage the input (the reference rotates in place / through a temporary)
            const size_t w = (size_t)(level + 1) * N;
            TRY(r->ctx->arena_reserve(B * w + 64));
            View tmp{r->ctx->arena_take(B * w), w};
            HIP_TRY(launch_ew(r->dev, tab, EW_COPY, v[0], v[0], tmp, B, nullptr, nullptr, r->ctx->stream));
            in = tmp;
        }
        if (monomial) HIP_TRY(launch_mult_by_monomial(r->dev, tab, in, kk, v[1], B, r->ctx->stream));
        else HIP_TRY(launch_shift(r->dev, tab, in, kk, v[1], B, r->ctx->stream));
        return HE_OK;
    };
    return co_dispatch(*r->ctx, batch, q);
}
int he_shift(he_handle r, int l, he_handle p1, int k, he_handle p2) { return shift_api(r, l, p1, k, p2, false, "he_shift"); }
int he_mult_by_monomial(he_handle r, int l, he_handle p1, int k, he_handle p2) { return shift_api(r, l, p1, k, p2, true, "he_mult_by_monomial"); }
int he_mul_by_vector_montgomery(he_handle hring, int level, he_handle h1, he_handle hv, int then_add_lazy, he_handle h2) {
    GET(r, Ring, hring, T_RING);
    const char *who = "he_mul_by_vector_montgomery";
    TRY(check_level(*r, level, who));
    CoReq q;
    Operands o(q, who, *r);
    o.in(hv, 1, "the vector (one batch-1 limb of degree N)", 1);
    const int i1 = o.in(h1, level + 1), i2 = o.out(h2, level + 1);
    o.inplace(i2, i1);  // p2 == vector is not in place: limb 0 of the output is the vector every other limb still reads
    TRY(o.check());
    q.ops[0].bstride = 0;  // the same vector for every batch entry and (through the limb override) every limb
    q.op = CO_EW; q.obj = r.get(); q.par[0] = level; q.par[1] = then_add_lazy ? EW_MUL_MONT_THEN_ADD_LAZY : EW_MUL_MONT; q.par[2] = 2;  // (a vector form)
    q.keep.push_back(r);
    q.run = [r, level, then_add_lazy](const View *w, int B) -> int {
        const uint8_t zeros[kMaxLimbs] = {0};
        r->ctx->acct((then_add_lazy ? 3.0 : 2.0) * (level + 1), 1.0, B, r->N);
        { Valu V(r->logN); for (int i = 0; i <= level; i++) V.mul(cls_f64(r->small, i), 1.0); V.into(*r->ctx, B); }
        HIP_TRY(launch_ew(r->dev, ident_tab(level + 1), then_add_lazy ? EW_MUL_MONT_THEN_ADD_LAZY : EW_MUL_MONT, w[0], w[1], w[2], B, nullptr,
                          zeros, r->ctx->stream));
        return HE_OK;
    };
    return co_dispatch(*r->ctx, o.B, q);
}
int he_add_scalar_bigint(he_handle r, int l, he_handle p1, const uint64_t *w, int n, he_handle p2) { return bigint_api(r, l, p1, w, n, p2, 0); }
int he_sub_scalar_bigint(he_handle r, int l, he_handle p1, const uint64_t *w, int n, he_handle p2) { return bigint_api(r, l, p1, w, n, p2, 1); }
int he_mul_scalar_bigint(he_handle r, int l, he_handle p1, const uint64_t *w, int n, he_handle p2) { return bigint_api(r, l, p1, w, n, p2, 2); }

int he_add(he_handle r, int l, he_handle a, he_handle b, he_handle c) { return he_binop(r, l, HE_ADD, a, b, c); }
int he_sub(he_handle r, int l, he_handle a, he_handle b, he_handle c) { return he_binop(r, l, HE_SUB, a, b, c); }
int he_neg(he_handle r, int l, he_handle a, he_handle b) { return he_unop(r, l, HE_NEG, a, b); }
int he_reduce(he_handle r, int l, he_handle a, he_handle b) { return he_unop(r, l, HE_REDUCE, a, b); }
int he_mform(he_handle r, int l, he_handle a, he_handle b) { return he_unop(r, l, HE_MFORM, a, b); }
int he_imform(he_handle r, int l, he_handle a, he_handle b) { return he_unop(r, l, HE_IMFORM, a, b); }
int he_mul_coeffs_montgomery(he_handle r, int l, he_handle a, he_handle b, he_handle c) { return he_binop(r, l, HE_MUL_COEFFS_MONTGOMERY, a, b, c); }
int he_mul_coeffs_montgomery_then_add(he_handle r, int l, he_handle a, he_handle b, he_handle c) { return he_binop(r, l, HE_MUL_COEFFS_MONTGOMERY_THEN_ADD, a, b, c); }
int he_mul_coeffs_montgomery_lazy(he_handle r, int l, he_handle a, he_handle b, he_handle c) { return he_binop(r, l, HE_MUL_COEFFS_MONTGOMERY_LAZY, a, b, c); }
int he_mul_coeffs_montgomery_lazy_then_add_lazy(he_handle r, int l, he_handle a, he_handle b, he_handle c) { return he_binop(r, l, HE_MUL_COEFFS_MONTGOMERY_LAZY_THEN_ADD_LAZY, a, b, c); }

// ---------------------------------------------------------------------------------------
// rescale (ring/scaling.go).  `mod0` lets the same routine run on a sub-chain.
// ---------------------------------------------------------------------------------------
namespace {
struct RescaleScratch {
    View s0;  // [batch][1][N]
    View s1;  // [batch][level][N]
};
// one DivRound/DivFloor step in the NTT domain: p0 (level+1 limbs) -> p1 (level limbs)
int div_by_last_modulus_ntt(Ring &r, int level, View p0, View p1, int batch, bool round, RescaleScratch sc) {
    hipStream_t st = r.ctx->stream;
    const int N = r.N;
    (void)N;
    // b0 = INTTLazy(p0[level])                                                  scaling.go:15 / :110
    LimbTab t_top;
    t_top.n = 1; t_top.in_limb[0] = (uint8_t)level; t_top.out_limb[0] = 0; t_top.mod[0] = (uint8_t)level;
    const uint64_t qL = r.moduli[level], phalf = (qL - 1) >> 1;
    if (r.type == 0) {
        // standard ring: the whole step is two transforms.  (1) b0 = CRed(INTT(p0[level]) + pHalf): the scalar rides on the
        // inverse's last pass.  (2) one forward transform per remaining modulus that reads b0, adds q_i - (pHalf mod q_i)
        // while loading, and applies MRed(. + 2q_i - p0_i, RescaleConstants) while storing.   scaling.go:110-120 (:15-24 floor)
        uint64_t s_in[kMaxLimbs], s_top[1] = {phalf};
        HIP_TRY(launch_ntt(r.dev, t_top, p0, sc.s0, batch, true, NTT_REDUCE_INPUT, st, round ? s_top : nullptr));
        if (level == 0) return HE_OK;
        LimbTab tin = ident_tab(level);
        NttEpilogue ep;
        for (int i = 0; i < level; i++) {
            const ModConst &m = r.sub[i].mc;
            tin.in_limb[i] = 0;
            s_in[i] = round ? m.q - bred_add(phalf, m.q, m.brc0) : 0;
            ep.s[i] = r.rescale[level - 1][i];
        }
        ep.y = p0; ep.has_w = false; ep.y_reduce = true;
        ep.has_dst = true; ep.dst = p1;
        HIP_TRY(launch_ntt(r.dev, tin, sc.s0, sc.s1, batch, false, NTT_REDUCE_INPUT | NTT_LAZY_OUT, st, round ? s_in : nullptr, &ep));
        return HE_OK;
    }
    // conjugate-invariant ring: the lazy representative of INTTConjugateInvariantLazy is observable in the other moduli -- exact words
    HIP_TRY(launch_ci_intt_lazy_ref(r.dev, r.sub[level].mc, level, View{p0.p + (size_t)level * r.N, p0.bstride, p0.tab}, sc.s0, batch, st));
    ScalarTab s{};
    if (round) {  // b0 += pHalf mod q_L                                          scaling.go:114
        LimbTab t0; t0.n = 1; t0.in_limb[0] = 0; t0.out_limb[0] = 0; t0.mod[0] = (uint8_t)level;
        s.s[0] = phalf;
        HIP_TRY(launch_ew(r.dev, t0, EW_ADD_SCALAR, sc.s0, sc.s0, sc.s0, batch, &s, nullptr, st));
    }
    if (level == 0) return HE_OK;
    // b1_i = b0 + (q_i - pHalf mod q_i)  (lazy), NTTLazy_i                       scaling.go:117-119
    LimbTab tl = ident_tab(level);
    uint8_t xl[kMaxLimbs] = {0};
    LimbTab tin = tl;
    for (int i = 0; i < level; i++) tin.in_limb[i] = 0;
    if (round) {
        for (int i = 0; i < level; i++) {
            const ModConst &m = r.sub[i].mc;
            s.s[i] = m.q - bred_add(phalf, m.q, m.brc0);
        }
        HIP_TRY(launch_ew(r.dev, tin, EW_ADD_SCALAR_LAZY, sc.s0, sc.s0, sc.s1, batch, &s, xl, st));
        HIP_TRY(ring_ntt(r, tl, sc.s1, sc.s1, batch, false, NTT_REDUCE_INPUT | NTT_LAZY_OUT));
    } else {
        HIP_TRY(ring_ntt(r, tin, sc.s0, sc.s1, batch, false, NTT_REDUCE_INPUT | NTT_LAZY_OUT));
    }
    // p1_i = MRed(b1_i + 2q_i - p0_i, RescaleConstants[level-1][i])             scaling.go:120
    for (int i = 0; i < level; i++) s.s[i] = r.rescale[level - 1][i];
    // x = s1 (limb i), y = p0 (limb i), z = p1 (limb i)
    HIP_TRY(launch_ew(r.dev, tl, EW_SUB_THEN_MUL_SCALAR_MONT_2Q, sc.s1, p0, p1, batch, &s, nullptr, st));
    return HE_OK;
}
// coefficient-domain step                                                         scaling.go:26-34, :126-144
int div_by_last_modulus_coeff(Ring &r, int level, View p0, View p1, int batch, bool round, RescaleScratch sc) {
    hipStream_t st = r.ctx->stream;
    if (level == 0) return HE_OK;
    ScalarTab s{};
    LimbTab tl = ident_tab(level);
    uint8_t xl[kMaxLimbs];
    if (round) {
        const uint64_t qL = r.moduli[level], phalf = (qL - 1) >> 1;
        LimbTab t0; t0.n = 1; t0.in_limb[0] = (uint8_t)level; t0.out_limb[0] = 0; t0.mod[0] = (uint8_t)level;
        s.s[0] = phalf;
        HIP_TRY(launch_ew(r.dev, t0, EW_ADD_SCALAR, p0, p0, sc.s0, batch, &s, nullptr, st));
        for (int i = 0; i < level; i++) {
            const ModConst &m = r.sub[i].mc;
            s.s[i] = r.rescale[level - 1][i];
            s.s2[i] = m.q - bred_add(phalf, m.q, m.brc0);
            xl[i] = 0;
        }
        HIP_TRY(launch_ew(r.dev, tl, EW_DIVROUND_COEFF, sc.s0, p0, p1, batch, &s, xl, st));
    } else {
        for (int i = 0; i < level; i++) { s.s[i] = r.rescale[level - 1][i]; xl[i] = (uint8_t)level; }
        HIP_TRY(launch_ew(r.dev, tl, EW_SUB_THEN_MUL_SCALAR_MONT_2Q, p0, p0, p1, batch, &s, xl, st));
    }
    return HE_OK;
}
// many: the *Many* entry points.  DivFloorByLastModulusManyNTT always goes INTT -> coefficient-domain steps -> NTT, even for one
// step (scaling.go:37-62), whereas DivRoundByLastModulusManyNTT(1) is DivRoundByLastModulusNTT (:169-171); on a standard ring
// the two routes give the same words, on a conjugate-invariant ring the single-step NTT form sees the lazy INTT words.
// the request of one DivRound / DivFloor call (validation + launches); div_many files it, he_rescale_polys files several at once
int div_fill(CoReq &q, const std::shared_ptr<Ring> &r, int level, int nb, he_handle h0, he_handle h1, bool round, bool ntt, const char *who,
             bool many, int *batch) {
    TRY(check_level(*r, level, who));
    if (nb < 0 || nb > level) return fail(HE_EINVAL, "%s: cannot divide %d times at level %d", who, nb, level);
    Operands o(q, who, *r);
    const int i0 = o.in(h0, level + 1), i1 = o.out(h1, level + 1 - nb);
    o.all_inplace = true;
    TRY(o.check());
    const bool same = o.same(i0, i1);
    *batch = o.B;
    q.op = CO_RESCALE; q.obj = r.get(); q.par[0] = level; q.par[1] = nb; q.par[2] = round; q.par[3] = ntt; q.par[4] = many;
    q.keep.push_back(r);
    q.run = [r, level, nb, round, ntt, many, same](const View *v, int B) -> int {
        for (int i = 0; i < nb; i++) r->ctx->acct(2.0 * (level - i + 1) - 1.0, 0, B, r->N);  // rescale: (2 L - 1) per polynomial and step
        {   // NTT form, one step: INTT of the top limb, one NTT and one product per remaining limb; otherwise: [INTT] + a product per
            // remaining limb and step + [NTT]
            Valu V(r->logN);
            if (ntt && nb == 1) { V.ntt(cls_f64(r->small, level)); for (int i = 0; i < level; i++) { V.ntt(cls_f64(r->small, i)); V.mul(cls_f64(r->small, i), 1.0); } }
            else {
                if (ntt) for (int i = 0; i <= level; i++) V.ntt(cls_f64(r->small, i));
                for (int st = 0; st < nb; st++) for (int i = 0; i < level - st; i++) V.mul(cls_f64(r->small, i), 1.0);
                if (ntt) for (int i = 0; i <= level - nb; i++) V.ntt(cls_f64(r->small, i));
            }
            V.into(*r->ctx, B);
        }
        hipStream_t st = r->ctx->stream;
        const int N = r->N;
        if (nb == 0) {
            if (!same) HIP_TRY(launch_ew(r->dev, ident_tab(level + 1), EW_COPY, v[0], v[0], v[1], B, nullptr, nullptr, st));
            return HE_OK;
        }
        const size_t w0 = (size_t)B * N, w1 = (size_t)B * (level + 1) * N;
        TRY(r->ctx->arena_reserve(w0 + 2 * w1));
        RescaleScratch rs;
        rs.s0 = View{r->ctx->arena_take(w0), (size_t)N};
        rs.s1 = View{r->ctx->arena_take(w1), (size_t)(level + 1) * N};
        if (ntt && nb == 1 && !(many && !round && r->type == 1)) return div_by_last_modulus_ntt(*r, level, v[0], v[1], B, round, rs);
        View buf{r->ctx->arena_take(w1), (size_t)(level + 1) * N};
        View cur = v[0];
        int lv = level;
        if (ntt) {  // INTT, nb coefficient-domain steps, NTT          scaling.go:37-62, :148-174
            HIP_TRY(ring_ntt(*r, ident_tab(level + 1), v[0], buf, B, true, NTT_REDUCE_INPUT));
            cur = buf;
        }
        for (int i = 0; i < nb; i++) {
            const bool last = (i == nb - 1);
            View dst = (last && !ntt) ? v[1] : buf;
            TRY(div_by_last_modulus_coeff(*r, lv, cur, dst, B, round, rs));
            cur = dst;
            lv--;
        }
        if (ntt) HIP_TRY(ring_ntt(*r, ident_tab(lv + 1), buf, v[1], B, false, NTT_REDUCE_INPUT));
        return HE_OK;
    };
    q.tables_ok = [r](bool *ok) -> int { *ok = r->type == 0; return HE_OK; };  // (conjugate-invariant rings: launches without entry tables)
    return HE_OK;
}
int div_many(he_handle hring, int level, int nb, he_handle h0, he_handle h1, bool round, bool ntt, const char *who, bool many = false) {
    GET(r, Ring, hring, T_RING);
    CoReq q;
    int B = 0;
    TRY(div_fill(q, r, level, nb, h0, h1, round, ntt, who, many, &B));
    return co_dispatch(*r->ctx, B, q);
}
}  // namespace

int he_div_round_by_last_modulus_ntt(he_handle r, int l, he_handle a, he_handle b) { return div_many(r, l, 1, a, b, true, true, "he_div_round_by_last_modulus_ntt"); }
int he_div_round_by_last_modulus(he_handle r, int l, he_handle a, he_handle b) { return div_many(r, l, 1, a, b, true, false, "he_div_round_by_last_modulus"); }
int he_div_floor_by_last_modulus_ntt(he_handle r, int l, he_handle a, he_handle b) { return div_many(r, l, 1, a, b, false, true, "he_div_floor_by_last_modulus_ntt"); }
int he_div_floor_by_last_modulus(he_handle r, int l, he_handle a, he_handle b) { return div_many(r, l, 1, a, b, false, false, "he_div_floor_by_last_modulus"); }
int he_div_round_by_last_modulus_many_ntt(he_handle r, int l, int nb, he_handle a, he_handle b) { return div_many(r, l, nb, a, b, true, true, "he_div_round_by_last_modulus_many_ntt"); }
int he_div_round_by_last_modulus_many(he_handle r, int l, int nb, he_handle a, he_handle b) { return div_many(r, l, nb, a, b, true, false, "he_div_round_by_last_modulus_many"); }
int he_div_floor_by_last_modulus_many_ntt(he_handle r, int l, int nb, he_handle a, he_handle b) { return div_many(r, l, nb, a, b, false, true, "he_div_floor_by_last_modulus_many_ntt", true); }
int he_div_floor_by_last_modulus_many(he_handle r, int l, int nb, he_handle a, he_handle b) { return div_many(r, l, nb, a, b, false, false, "he_div_floor_by_last_modulus_many"); }
// Evaluator.Rescale's loop over the polynomials of a ciphertext (schemes/ckks/evaluator.go:503-507, schemes/bgv/evaluator.go:
// 1385-1389: DivRoundByLastModulusManyNTT per component) as ONE call: on a context whose queue is on, the n requests are filed
// together and share a batch with the other callers' -- a degree-2 ciphertext's Rescale is one round of the queue, not three.
int he_rescale_polys(he_handle hring, int level, int nb, int n, const he_handle *p0, const he_handle *p1) {
    GET(r, Ring, hring, T_RING);
    if (n < 0 || n > 16 || (n > 0 && (!p0 || !p1))) return fail(HE_EINVAL, "he_rescale_polys: n in [0, 16] and both handle arrays");
    std::deque<CoReq> qs((size_t)n);
    std::vector<CoReq *> ptrs;
    const int max_batch = r->ctx->co->max_batch.load(std::memory_order_relaxed);
    bool queue = max_batch > 1 && !r->ctx->capturing;
    for (int i = 0; i < n; i++) {
        int B = 0;
        TRY(div_fill(qs[i], r, level, nb, p0[i], p1[i], true, true, "he_rescale_polys", false, &B));
        queue = queue && B >= 1 && B < max_batch;
        qs[i].nb = B;
        ptrs.push_back(&qs[i]);
    }
    // each pair may be in place; an output that is an operand of ANOTHER pair is not (the queue files the n pairs as one batch, the
    // direct path runs them one after the other: the two would differ).  Same polynomial = same device storage, as reject_aliasing.
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            const uint64_t *o = qs[i].ops[1].p;
            if (i != j && (o == qs[j].ops[0].p || (i < j && o == qs[j].ops[1].p)))
                return fail(HE_EINVAL, "he_rescale_polys: output %d is also %s %d", i, o == qs[j].ops[0].p ? "input" : "output", j);
        }
    if (n == 0) return HE_OK;
    if (queue) {
        for (CoReq &q : qs) q.set_alias_pattern();
        return co_submit_many(*r->ctx, ptrs);
    }
    for (int i = 0; i < n; i++) {
        int B = 0;
        GET(pp, Poly, p0[i], T_POLY);
        B = pp->batch;
        Scope sc(r->ctx.get());
        TRY(qs[i].run(qs[i].ops.data(), B));
    }
    return HE_OK;
}

// ---------------------------------------------------------------------------------------
// automorphism (ring/automorphism.go)
// ---------------------------------------------------------------------------------------
int he_automorphism_index_create(he_handle hring, uint64_t gal, he_handle *out) {
    GET(r, Ring, hring, T_RING);
    if (!out || !(gal & 1)) return fail(HE_EINVAL, "he_automorphism_index_create: Galois element must be odd");
    gal = reduce_gal(gal, r->logN, r->type);
    auto ix = std::make_shared<AutoIndex>();
    ix->ctx = r->ctx;
    ix->N = r->N;
    ix->gal = gal;
    {
        std::lock_guard<std::mutex> lk(r->index_mu);
        auto it = r->index_cache.find(gal);
        if (it != r->index_cache.end()) ix->tab = it->second;
    }
    if (!ix->tab) {
        auto tab = std::make_shared<IndexTable>();
        tab->ctx = r->ctx;
        {
            Scope sc(r->ctx.get());
            HIP_TRY(hipMalloc((void **)&tab->d, (size_t)r->N * sizeof(uint32_t)));
            HIP_TRY(launch_build_automorphism_index(r->logN, r->logN + r->type, gal, tab->d, r->ctx->stream));
        }
        std::lock_guard<std::mutex> lk(r->index_mu);
        auto it = r->index_cache.find(gal);
        if (it != r->index_cache.end()) tab = it->second;  // (another thread built it meanwhile: one table per element)
        else if (r->index_cache.size() < Ring::kIndexCacheCap) r->index_cache.emplace(gal, tab);
        ix->tab = tab;
    }
    ix->d = ix->tab->d;
    *out = reg(ix);
    return HE_OK;
}
int he_automorphism_index_destroy(he_handle h) { return unreg(h, T_INDEX); }
int he_automorphism_index_download(he_handle h, uint64_t *dst) {
    GET(ix, AutoIndex, h, T_INDEX);
    if (!dst) return fail(HE_EINVAL, "he_automorphism_index_download: null destination");
    std::vector<uint32_t> tmp(ix->N);
    Scope sc(ix->ctx.get());
    HIP_TRY(hipMemcpyAsync(tmp.data(), ix->d, (size_t)ix->N * 4, hipMemcpyDeviceToHost, ix->ctx->stream));
    HIP_TRY(hipStreamSynchronize(ix->ctx->stream));
    for (int i = 0; i < ix->N; i++) dst[i] = tmp[i];
    return HE_OK;
}
static int gather_api(he_handle hring, int level, he_handle hin, he_handle hidx, he_handle hout, bool add, const char *who) {
    GET(r, Ring, hring, T_RING);
    GET(ix, AutoIndex, hidx, T_INDEX);
    TRY(check_level(*r, level, who));
    if (ix->N != r->N) return fail(HE_EINVAL, "%s: shape mismatch", who);
    CoReq q;
    Operands o(q, who, *r);
    o.in(hin, level + 1);
    o.out(hout, level + 1);
    TRY(o.check());  // (never in place, ring/automorphism.go:37)
    // (the index table is identified by its Galois element, not by its handle: callers that each built their own table of the same
    // automorphism share a batch -- entry 0's table serves them all)
    // ... and by the cached table it points at: handles built on rings of another type (standard / conjugate-invariant, another
    // NthRoot) with the same N and Galois element hold a different permutation and must not share entry 0's table
    q.op = CO_GATHER; q.obj = r.get(); q.par[0] = level; q.par[1] = add; q.par[2] = (int64_t)ix->gal; q.par[3] = (int64_t)(uintptr_t)ix->d;
    q.keep.push_back(r); q.keep.push_back(ix);
    q.run = [r, ix, level, add](const View *v, int B) -> int {
        r->ctx->acct((add ? 3.0 : 2.0) * (level + 1), 0, B, r->N);  // automorphism: 2 L (+ L for ...ThenAddLazy)
        HIP_TRY(launch_gather(r->dev, ident_tab(level + 1), v[0], ix->d, v[1], B, add, r->ctx->stream));
        return HE_OK;
    };
    return co_dispatch(*r->ctx, o.B, q);
}
int he_automorphism_ntt_with_index(he_handle r, int l, he_handle in, he_handle idx, he_handle out) { return gather_api(r, l, in, idx, out, false, "he_automorphism_ntt_with_index"); }
int he_automorphism_ntt_with_index_then_add_lazy(he_handle r, int l, he_handle in, he_handle idx, he_handle out) { return gather_api(r, l, in, idx, out, true, "he_automorphism_ntt_with_index_then_add_lazy"); }
int he_automorphism(he_handle hring, int level, he_handle hin, uint64_t gal, he_handle hout) {
    GET(r, Ring, hring, T_RING);
    TRY(check_level(*r, level, "he_automorphism"));
    CoReq q;
    Operands o(q, "he_automorphism", *r);
    o.in(hin, level + 1);
    o.out(hout, level + 1);
    TRY(o.check());  // (never in place)
    gal = reduce_gal(gal, r->logN, r->type);
    q.op = CO_AUTO_COEFF; q.obj = r.get(); q.par[0] = level; q.par[1] = (int64_t)gal;
    q.keep.push_back(r);
    q.run = [r, level, gal](const View *v, int B) -> int {
        r->ctx->acct(2.0 * (level + 1), 0, B, r->N);
        HIP_TRY(launch_automorphism_coeff(r->dev, ident_tab(level + 1), v[0], gal, v[1], B, r->ctx->stream, r->type == 1));
        return HE_OK;
    };
    return co_dispatch(*r->ctx, o.B, q);
}

// ---------------------------------------------------------------------------------------
// basis extension (ring/basis_extension.go)
// ---------------------------------------------------------------------------------------
// P may be a ring without moduli (an evaluator over parameters without special primes): LP = 0, no constants
static int basis_extender_build(std::shared_ptr<Ring> Q, std::shared_ptr<Ring> P, he_handle *out) {
    if (Q->ctx != P->ctx || Q->N != P->N) return fail(HE_EINVAL, "he_basis_extender_create: rings must share context and degree");
    if (P->nmod() > 0 && Q->type != P->type) return fail(HE_EINVAL, "he_basis_extender_create: Q and P must be of the same ring type");
    if (Q->nmod() + P->nmod() > kMaxLimbs) return fail(HE_EINVAL, "he_basis_extender_create: more than %d moduli in QP", kMaxLimbs);
    if (Q->nmod() > 32 || P->nmod() > 32) return fail(HE_EINVAL, "he_basis_extender_create: at most 32 source limbs (ring/basis_extension.go:285)");
    for (uint64_t q : Q->moduli)
        for (uint64_t p : P->moduli)
            if (q == p) return fail(HE_EPARAM, "he_basis_extender_create: Q and P share a modulus");
    auto be = std::make_shared<BasisExtender>();
    be->ctx = Q->ctx; be->Q = Q; be->P = P; be->LQ = Q->nmod(); be->LP = P->nmod(); be->type = Q->type;
    Scope sc(Q->ctx.get());
    std::vector<const SubRingHost *> subs;
    for (auto &s : Q->sub) subs.push_back(&s);
    for (auto &s : P->sub) subs.push_back(&s);
    TRY(upload_tables(subs, Q->N, &be->d_mc, &be->d_twf, &be->d_twi));
    for (uint64_t m : Q->moduli) be->small.push_back(modulus_class(m));
    for (uint64_t m : P->moduli) be->small.push_back(modulus_class(m));
    TRY(upload_f64_tables(subs, Q->N, &be->d_twdf, &be->d_twdi));
    be->qp = RingDev{Q->logN, Q->N, be->d_mc, be->d_twf, be->d_twi, be->small.data(), be->d_twdf, be->d_twdi};
    {   // Shoup pairs of the first sixteen forward twiddles (the column stages fused into the basis extension)
        std::vector<uint64_t> tws(subs.size() * 32, 0);
        for (size_t i = 0; i < subs.size(); i++) {
            const ModConst &m = subs[i]->mc;
            for (int j = 0; j < 16 && j < Q->N; j++) {
                const uint64_t w = imform(subs[i]->roots_fwd[j], m.q, m.qinv);
                tws[i * 32 + 2 * j] = w;
                tws[i * 32 + 2 * j + 1] = (uint64_t)(((u128)w << 64) / m.q);
            }
        }
        HIP_TRY(hipMalloc((void **)&be->d_tws, tws.size() * 8));
        HIP_TRY(hipMemcpy(be->d_tws, tws.data(), tws.size() * 8, hipMemcpyHostToDevice));
        be->qp.tws_fwd = be->d_tws;
    }
    for (int i = 0; i < be->LQ; i++)  // constantsQtoP[i] = GenModUpConstants(Q[:i+1], P)     basis_extension.go:62-65
        be->qtop.push_back(pool_modup(be->pool, std::vector<uint64_t>(Q->moduli.begin(), Q->moduli.begin() + i + 1), P->moduli));
    for (int i = 0; i < be->LP; i++)  // constantsPtoQ[i] = GenModUpConstants(P[:i+1], Q)     :67-70
        be->ptoq.push_back(pool_modup(be->pool, std::vector<uint64_t>(P->moduli.begin(), P->moduli.begin() + i + 1), Q->moduli));
    TRY(be->pool.upload());
    be->md_ptoq.resize(be->LP);
    for (int j = 0; j < be->LP; j++) {
        std::vector<uint64_t> S(P->moduli.begin(), P->moduli.begin() + j + 1);
        for (int i = 0; i < be->LQ; i++) be->md_ptoq[j].push_back(inv_product_mont(S, Q->moduli[i]));
    }
    be->md_qtop.resize(be->LQ);
    for (int j = 0; j < be->LQ; j++) {
        std::vector<uint64_t> S(Q->moduli.begin(), Q->moduli.begin() + j + 1);
        for (int i = 0; i < be->LP; i++) be->md_qtop[j].push_back(inv_product_mont(S, P->moduli[i]));
    }
    *out = reg(be);
    return HE_OK;
}
int he_basis_extender_create(he_handle hq, he_handle hp, he_handle *out) {
    GET(Q, Ring, hq, T_RING);
    GET(P, Ring, hp, T_RING);
    if (!out) return fail(HE_EINVAL, "he_basis_extender_create: null output");
    return basis_extender_build(Q, P, out);
}
int he_basis_extender_destroy(he_handle h) { return unreg(h, T_BE); }

namespace {
// multSum's result stays below 4*p only while nsrc * max(source modulus) < 2^64; beyond that the
// following forward NTT must first bring its input back to [0,2q).
bool modup_out_needs_reduce(const std::vector<uint64_t> &basis) {
    uint64_t mx = 0;
    for (uint64_t m : basis) mx = std::max(mx, m);
    return ((u128)mx * basis.size()) >> 63 != 0;
}
// ModUpQtoP / ModUpPtoQ (basis_extension.go:177-210): src limbs [0..levelS] of the source
// ring -> dst limbs [0..levelD] of the other ring, centred by floor(S/2).
// src_is_q selects direction.  dst_limb0 / dst view allow writing into QP-contiguous scratch.
int modup_between(BasisExtender &be, bool src_is_q, int levelS, int levelD, View src, View dst, int dst_limb0, int batch) {
    const Ring &S = src_is_q ? *be.Q : *be.P;
    const Ring &D = src_is_q ? *be.P : *be.Q;
    const int smod0 = src_is_q ? 0 : be.LQ, dmod0 = src_is_q ? be.LQ : 0;
    const ModUpRef &ref = src_is_q ? be.qtop[levelS] : be.ptoq[levelS];
    std::vector<uint64_t> basis(S.moduli.begin(), S.moduli.begin() + levelS + 1);
    ModUpArgs a{};
    a.nsrc = levelS + 1;
    a.ndst = levelD + 1;
    for (int i = 0; i <= levelS; i++) {
        a.src_limb[i] = (uint8_t)i;
        a.src_mod[i] = (uint8_t)(smod0 + i);
        a.src_half[i] = half_product_mod(basis, S.moduli[i]);
    }
    for (int j = 0; j <= levelD; j++) {
        a.dst_limb[j] = (uint8_t)(dst_limb0 + j);
        a.dst_mod[j] = (uint8_t)(dmod0 + j);
        a.dst_row[j] = (uint8_t)j;
        a.dst_half[j] = half_product_mod(basis, D.moduli[j]);
        a.dst_view[j] = 0;
    }
    HIP_TRY(launch_modup(be.qp, ref.on(be.pool), a, src, dst, dst, batch, be.ctx->stream));
    return HE_OK;
}
// ModDownQPtoQNTT for `batch` entries (basis_extension.go:235-256); pQ/pP NTT domain in, outQ NTT out.
// scratch: sP [batch][levelP+1][N], sQ [batch][levelQ+1][N]
int moddown_q_ntt(BasisExtender &be, int levelQ, int levelP, View pQ, View pP, View outQ, int batch, View sP, View sQ) {
    hipStream_t st = be.ctx->stream;
    // ringP.INTTLazy(p1P, buffP)
    HIP_TRY(be_ntt(be, ident_tab(levelP + 1, 0, 0, be.LQ), pP, sP, batch, true, NTT_REDUCE_INPUT));
    // ModUpPtoQ(buffP) -> buffQ
    TRY(modup_between(be, false, levelP, levelQ, sP, sQ, 0, batch));
    // ringQ.NTTLazy(buffQ, buffQ)
    const bool red = modup_out_needs_reduce(std::vector<uint64_t>(be.P->moduli.begin(), be.P->moduli.begin() + levelP + 1));
    HIP_TRY(be_ntt(be, ident_tab(levelQ + 1), sQ, sQ, batch, false, NTT_LAZY_OUT | (red ? NTT_REDUCE_INPUT : 0)));
    // p2Q_i = MRed(buffQ_i + 2q_i - p1Q_i, q_i - modDownConstants[i])
    ScalarTab s{};
    for (int i = 0; i <= levelQ; i++) s.s[i] = be.Q->moduli[i] - be.md_ptoq[levelP][i];
    HIP_TRY(launch_ew(be.qp, ident_tab(levelQ + 1), EW_SUB_THEN_MUL_SCALAR_MONT_2Q, sQ, pQ, outQ, batch, &s, nullptr, st));
    return HE_OK;
}
}  // namespace

int he_modup_q_to_p(he_handle hbe, int levelQ, int levelP, he_handle hq, he_handle hp) {
    GET(be, BasisExtender, hbe, T_BE);
    if (levelQ < 0 || levelQ >= be->LQ || levelP < 0 || levelP >= be->LP) return fail(HE_EINVAL, "he_modup_q_to_p: level out of range");
    CoReq q;
    Operands o(q, "he_modup_q_to_p", *be);
    o.in(hq, levelQ + 1);
    o.outP(hp, levelP + 1);
    TRY(o.check());
    q.op = CO_MODUP; q.obj = be.get(); q.par[0] = levelQ; q.par[1] = levelP; q.par[2] = 1;
    q.keep.push_back(be);
    q.run = [be, levelQ, levelP](const View *v, int B) -> int {
        be->ctx->acct(levelQ + 1 + levelP + 1, 0, B, be->Q->N);  // ModUp: L_src + L_dst
        { Valu V(be->Q->logN); std::vector<int> d; for (int j = 0; j <= levelP; j++) d.push_back(be->LQ + j); valu_modup(V, be->small, 0, levelQ + 1, d); V.into(*be->ctx, B); }
        return modup_between(*be, true, levelQ, levelP, v[0], v[1], 0, B);
    };
    return co_dispatch(*be->ctx, o.B, q);
}
int he_modup_p_to_q(he_handle hbe, int levelP, int levelQ, he_handle hp, he_handle hq) {
    GET(be, BasisExtender, hbe, T_BE);
    if (levelQ < 0 || levelQ >= be->LQ || levelP < 0 || levelP >= be->LP) return fail(HE_EINVAL, "he_modup_p_to_q: level out of range");
    CoReq q;
    Operands o(q, "he_modup_p_to_q", *be);
    o.inP(hp, levelP + 1);
    o.out(hq, levelQ + 1);
    TRY(o.check());
    q.op = CO_MODUP; q.obj = be.get(); q.par[0] = levelQ; q.par[1] = levelP; q.par[2] = 0;
    q.keep.push_back(be);
    q.run = [be, levelQ, levelP](const View *v, int B) -> int {
        be->ctx->acct(levelQ + 1 + levelP + 1, 0, B, be->Q->N);
        { Valu V(be->Q->logN); std::vector<int> d; for (int i = 0; i <= levelQ; i++) d.push_back(i); valu_modup(V, be->small, be->LQ, levelP + 1, d); V.into(*be->ctx, B); }
        return modup_between(*be, false, levelP, levelQ, v[0], v[1], 0, B);
    };
    return co_dispatch(*be->ctx, o.B, q);
}
static int moddown_api(he_handle hbe, int levelQ, int levelP, he_handle h1q, he_handle h1p, he_handle h2, int kind, const char *who) {
    GET(be, BasisExtender, hbe, T_BE);
    if (levelQ < 0 || levelQ >= be->LQ || levelP < 0 || levelP >= be->LP) return fail(HE_EINVAL, "%s: level out of range", who);
    CoReq q;
    Operands o(q, who, *be);
    const int iq = o.in(h1q, levelQ + 1), ip = o.inP(h1p, levelP + 1);
    // in place: p2Q == p1Q (ModDownQPtoQ[NTT]) or p2P == p1P (ModDownQPtoP), element-wise in the last launch
    if (kind == 2) o.inplace(o.outP(h2, levelP + 1), ip);
    else o.inplace(o.out(h2, levelQ + 1), iq);
    TRY(o.check());
    q.op = CO_MODDOWN_BE; q.obj = be.get(); q.par[0] = levelQ; q.par[1] = levelP; q.par[2] = kind;
    q.keep.push_back(be);
    q.run = [be, levelQ, levelP, kind](const View *v, int B) -> int {
        const int N = be->Q->N;
        be->ctx->acct(kind == 2 ? levelQ + 1 + 2.0 * (levelP + 1) : 2.0 * (levelQ + 1) + levelP + 1, 0, B, N);  // ModDown: 2 L + alpha
        {
            Valu V(be->Q->logN);
            if (kind != 2) valu_moddown(V, *be, levelQ, levelP, kind == 1);
            else { std::vector<int> d; for (int j = 0; j <= levelP; j++) { d.push_back(be->LQ + j); V.mul(cls_f64(be->small, be->LQ + j), 1.0); } valu_modup(V, be->small, 0, levelQ + 1, d); }
            V.into(*be->ctx, B);
        }
        const size_t wP = (size_t)B * (levelP + 1) * N, wQ = (size_t)B * (levelQ + 1) * N;
        TRY(be->ctx->arena_reserve(wP + wQ));
        View sP{be->ctx->arena_take(wP), (size_t)(levelP + 1) * N};
        View sQ{be->ctx->arena_take(wQ), (size_t)(levelQ + 1) * N};
        hipStream_t st = be->ctx->stream;
        ScalarTab s{};
        if (kind == 1) return moddown_q_ntt(*be, levelQ, levelP, v[0], v[1], v[2], B, sP, sQ);
        if (kind == 0) {  // ModDownQPtoQ, basis_extension.go:215-230
            TRY(modup_between(*be, false, levelP, levelQ, v[1], sQ, 0, B));
            for (int i = 0; i <= levelQ; i++) s.s[i] = be->Q->moduli[i] - be->md_ptoq[levelP][i];
            HIP_TRY(launch_ew(be->qp, ident_tab(levelQ + 1), EW_SUB_THEN_MUL_SCALAR_MONT_2Q, sQ, v[0], v[2], B, &s, nullptr, st));
            return HE_OK;
        }
        // ModDownQPtoP, basis_extension.go:262-277
        TRY(modup_between(*be, true, levelQ, levelP, v[0], sP, 0, B));
        for (int i = 0; i <= levelP; i++) s.s[i] = be->P->moduli[i] - be->md_qtop[levelQ][i];
        HIP_TRY(launch_ew(be->qp, ident_tab(levelP + 1, 0, 0, be->LQ), EW_SUB_THEN_MUL_SCALAR_MONT_2Q, sP, v[1], v[2], B, &s, nullptr, st));
        return HE_OK;
    };
    q.tables_ok = [be](bool *ok) -> int { *ok = be->type == 0; return HE_OK; };
    return co_dispatch(*be->ctx, o.B, q);
}
int he_moddown_qp_to_q(he_handle be, int lq, int lp, he_handle a, he_handle b, he_handle c) { return moddown_api(be, lq, lp, a, b, c, 0, "he_moddown_qp_to_q"); }
int he_moddown_qp_to_q_ntt(he_handle be, int lq, int lp, he_handle a, he_handle b, he_handle c) { return moddown_api(be, lq, lp, a, b, c, 1, "he_moddown_qp_to_q_ntt"); }
int he_moddown_qp_to_p(he_handle be, int lq, int lp, he_handle a, he_handle b, he_handle c) { return moddown_api(be, lq, lp, a, b, c, 2, "he_moddown_qp_to_p"); }

// ---------------------------------------------------------------------------------------
// rlwe.Evaluator
// ---------------------------------------------------------------------------------------
int he_evaluator_create(he_handle hq, he_handle hp, he_handle *out) {
    if (!out) return fail(HE_EINVAL, "he_evaluator_create: null output");
    he_handle hbe = 0;
    if (hp == 0) {
        // parameters without special primes (rlwe.ParametersLiteral.P = nil): levelP = -1 everywhere.  The evaluator then
        // serves base-2 gadget keys without a P part (the reference's own P-less set, core/rlwe/test_params.go:36-46) through
        // gadgetProductSinglePAndBitDecompLazy's `ringP == nil` branches and ModDown's `levelP == -1` copy.
        GET(Q, Ring, hq, T_RING);
        auto P = std::make_shared<Ring>();
        P->ctx = Q->ctx; P->logN = Q->logN; P->N = Q->N; P->type = 0;
        TRY(basis_extender_build(Q, P, &hbe));
    } else {
        TRY(he_basis_extender_create(hq, hp, &hbe));
    }
    auto be = get<BasisExtender>(hbe, T_BE);
    reg_drop(hbe);  // the evaluator owns its extender; drop the public handle
    auto ev = std::make_shared<Evaluator>();
    ev->be = be;
    const int LQ = be->LQ, LP = be->LP;
    const std::vector<uint64_t> &Q = be->Q->moduli, &P = be->P->moduli;
    // NewDecomposer (ring/basis_extension.go:320-377): for nbPi = 2..LP
    ev->dec.resize(LP > 1 ? LP - 1 : 0);
    for (int lvlP = 0; lvlP < LP - 1; lvlP++) {
        const int nbPi = lvlP + 2;
        const int nd = (LQ + nbPi - 1) / nbPi;
        ev->dec[lvlP].resize(nd);
        std::vector<uint64_t> D(Q);
        D.insert(D.end(), P.begin(), P.begin() + nbPi);
        for (int i = 0; i < nd; i++) {
            int xnb = nbPi;
            if (i == nd - 1 && LQ % nbPi != 0) xnb = LQ % nbPi;
            for (int j = 0; j < xnb - 1; j++) {
                std::vector<uint64_t> S(Q.begin() + i * nbPi, Q.begin() + i * nbPi + j + 2);
                ev->dec[lvlP][i].push_back(pool_modup(ev->pool, S, D));
            }
        }
    }
    Scope sc(be->ctx.get());
    TRY(ev->pool.upload());
    *out = reg(ev);
    return HE_OK;
}
int he_evaluator_destroy(he_handle h) { return unreg(h, T_EVAL); }
static int ctx_set_coalescing(const std::shared_ptr<Ctx> &c, int max_batch, int window_us, const char *who) {
    if (max_batch < 0 || max_batch > 1024 || window_us < 0 || window_us > 100000)
        return fail(HE_EINVAL, "%s: max_batch in [0, 1024], window_us in [0, 100000]", who);
    if (max_batch <= 1) co_stop_dispatcher(*c);  // (deferred submission ends with the queue: what is pending is launched first)
    else if (c->co->depth.load(std::memory_order_relaxed) > 0) TRY(co_flush_filed(*c));
    Scope sc(c.get());  // (a leader launches its batch under this lock: none is between gathering and launching while we hold it)
    Coalescer &co = *c->co;
    std::lock_guard<std::mutex> lk(co.mu);
    if (!co.pending.empty() || co.leader || co.n_deferred > 0) return fail(HE_EINVAL, "%s: calls are in flight on this context", who);
    if (max_batch <= 1) {  // off: later calls launch directly
        co.max_batch = 0;
        return HE_OK;
    }
    // rows for the operands of any call but the longest lintrans term lists (those are served one by one when they do not fit)
    const size_t words = (size_t)std::max<size_t>(kTabRowsMin, 128) * (size_t)max_batch;
    if (words > co.tab_words) {
        HIP_TRY(hipStreamSynchronize(c->stream));  // launches that read the old table
        if (co.d_tab) HIP_TRY(hipFree(co.d_tab));
        co.d_tab = nullptr; co.tab_words = 0;
        HIP_TRY(hipMalloc((void **)&co.d_tab, words * sizeof(size_t) * Coalescer::kTabSlots));
        co.tab_words = words;
        for (auto &sl : co.tab_slot) { sl.vals.clear(); sl.used = 0; }
    }
    co.max_batch = max_batch;
    co.window_us = window_us;
    return HE_OK;
}
static int ctx_coalescing_stats(Ctx &c, uint64_t out[4], const char *who) {
    if (!out) return fail(HE_EINVAL, "%s: null output", who);
    std::lock_guard<std::mutex> lk(c.co->mu);
    out[0] = c.co->n_calls; out[1] = c.co->n_launches; out[2] = c.co->n_max; out[3] = c.co->n_fallback;
    return HE_OK;
}
// the queue belongs to the context (round 5): the evaluator-level entry points of round 4 address their context's queue
int he_evaluator_set_coalescing(he_handle h, int max_batch, int window_us) {
    GET(ev, Evaluator, h, T_EVAL);
    return ctx_set_coalescing(ev->be->ctx, max_batch, window_us, "he_evaluator_set_coalescing");
}
int he_evaluator_coalescing_stats(he_handle h, uint64_t out[4]) {
    GET(ev, Evaluator, h, T_EVAL);
    return ctx_coalescing_stats(*ev->be->ctx, out, "he_evaluator_coalescing_stats");
}
int he_ctx_set_coalescing(he_handle h, int max_batch, int window_us) {
    GET(c, Ctx, h, T_CTX);
    return ctx_set_coalescing(c, max_batch, window_us, "he_ctx_set_coalescing");
}
int he_ctx_set_deferred(he_handle h, int depth) {
    GET(c, Ctx, h, T_CTX);
    if (depth < 0 || depth > 256) return fail(HE_EINVAL, "he_ctx_set_deferred: depth in [0, 256]");
    if (depth == 0) { co_stop_dispatcher(*c); return HE_OK; }
    Coalescer &co = *c->co;
    std::lock_guard<std::mutex> lk(co.mu);
    if (co.max_batch.load(std::memory_order_relaxed) <= 1)
        return fail(HE_EINVAL, "he_ctx_set_deferred: the submission queue is off (he_ctx_set_coalescing first)");
    if (co.stop) return fail(HE_EINVAL, "he_ctx_set_deferred: the dispatcher is being stopped");
    if (!co.dispatcher.joinable()) {
        if (!co.pending.empty() || co.leader) return fail(HE_EINVAL, "he_ctx_set_deferred: calls are in flight on this context");
        co.dispatcher = std::thread(co_dispatcher_main, c.get());
    }
    co.depth = depth;
    return HE_OK;
}
// a request whose launch fails after it was accepted (tests: where does the failure surface in each mode of the queue?)
int he_debug_queue_inject_failure(he_handle h) {
    GET(c, Ctx, h, T_CTX);
    CoReq q;
    q.op = 31; q.obj = c.get();
    q.keep = {c};
    q.run = [](const View *, int) -> int { return fail(HE_EDEVICE, "injected launch failure"); };
    return co_dispatch(*c, 1, q);
}
int he_debug_queue_op_stats(he_handle h, uint64_t out[64]) {
    GET(c, Ctx, h, T_CTX);
    if (!out) return fail(HE_EINVAL, "he_debug_queue_op_stats: null output");
    Scope sc(c.get());
    for (int i = 0; i < 32; i++) { out[2 * i] = c->co->op_launches[i]; out[2 * i + 1] = c->co->op_calls[i]; }
    return HE_OK;
}
int he_debug_queue_counters(he_handle h, uint64_t out[16]) {
    GET(c, Ctx, h, T_CTX);
    if (!out) return fail(HE_EINVAL, "he_debug_queue_counters: null output");
    std::lock_guard<std::mutex> lk(c->co->mu);
    for (int i = 0; i < 16; i++) out[i] = c->co->dbg[i];
    out[7] = c->pool_misses.load(std::memory_order_relaxed);
    out[13] = c->co->tab_fills; out[14] = c->co->tab_hits;  // (entry tables filled / reused; written under the context's lock: a glance)
    return HE_OK;
}
int he_ctx_coalescing_stats(he_handle h, uint64_t out[4]) {
    GET(c, Ctx, h, T_CTX);
    return ctx_coalescing_stats(*c, out, "he_ctx_coalescing_stats");
}

static int evk_derive(Evk &k) {
    BasisExtender &be = *k.ev->be;
    const int nQk = k.nQk, nPk = k.nPk;
    const size_t blk = (size_t)(nQk + nPk) * be.Q->N;
    bool any = false;
    uint8_t mods[kMaxLimbs];
    for (int i = 0; i < nQk; i++) { mods[i] = (uint8_t)i; any = any || be.small[i] == 2; }
    for (int i = 0; i < nPk; i++) { mods[nQk + i] = (uint8_t)(be.LQ + i); any = any || be.small[be.LQ + i] == 2; }
    if (any && be.d_twdf && k.pw2 == 0) {
        if (!k.keyd) HIP_TRY(hipMalloc((void **)&k.keyd, (size_t)k.beta * 2 * blk * 8));
        HIP_TRY(launch_key_to_f64(be.qp, k.d, k.keyd, k.beta * 2, mods, nQk + nPk, be.ctx->stream));
    }
    return HE_OK;
}

static int evk_create_common(he_handle hev, int beta, int nQk, int nPk, const uint64_t *q, const uint64_t *p, int pw2,
                             const int *nj, int n_rns, he_handle *out) {
    GET(ev, Evaluator, hev, T_EVAL);
    BasisExtender &be = *ev->be;
    const bool empty = !q;  // shape only: contents arrive through he_evk_device_buffer + he_evk_commit
    if ((!empty && (!q || (!p && nPk > 0))) || !out || beta <= 0 || nQk <= 0 || nQk > be.LQ || nPk < 0 || nPk > be.LP || (nPk == 0 && !pw2))
        return fail(HE_EINVAL, "he_evk_create: bad key shape (beta=%d, nQk=%d, nPk=%d)", beta, nQk, nPk);
    auto k = std::make_shared<Evk>();
    k->ev = ev; k->beta = beta; k->nQk = nQk; k->nPk = nPk; k->pw2 = pw2;
    if (pw2) {
        k->prefix.push_back(0);
        for (int i = 0; i < n_rns; i++) { k->nj.push_back(nj[i]); k->prefix.push_back(k->prefix.back() + nj[i]); }
    }
    Scope sc(be.ctx.get());
    const size_t N = be.Q->N, blk = (size_t)(nQk + nPk) * N;
    HIP_TRY(hipMalloc((void **)&k->d, (size_t)beta * 2 * blk * 8));
    if (empty) HIP_TRY(hipMemsetAsync(k->d, 0, (size_t)beta * 2 * blk * 8, be.ctx->stream));
    else
        for (int d = 0; d < beta; d++)
            for (int kk = 0; kk < 2; kk++) {
                uint64_t *dst = k->d + ((size_t)d * 2 + kk) * blk;
                HIP_TRY(hipMemcpyAsync(dst, q + ((size_t)d * 2 + kk) * nQk * N, (size_t)nQk * N * 8, hipMemcpyHostToDevice, be.ctx->stream));
                if (nPk > 0)
                    HIP_TRY(hipMemcpyAsync(dst + (size_t)nQk * N, p + ((size_t)d * 2 + kk) * nPk * N, (size_t)nPk * N * 8, hipMemcpyHostToDevice, be.ctx->stream));
            }
    if (int rc = evk_derive(*k)) return rc;
    HIP_TRY(hipStreamSynchronize(be.ctx->stream));
    *out = reg(k);
    return HE_OK;
}
int he_evk_create(he_handle hev, int beta, int nQk, int nPk, const uint64_t *q, const uint64_t *p, he_handle *out) {
    return evk_create_common(hev, beta, nQk, nPk, q, p, 0, nullptr, 0, out);
}
int he_evk_create_base2(he_handle hev, int pw2, const int *nj, int n_rns, int nQk, int nPk, const uint64_t *q, const uint64_t *p,
                        he_handle *out) {
    if (pw2 <= 0 || pw2 > 62 || !nj || n_rns != nQk) return fail(HE_EINVAL, "he_evk_create_base2: one RNS digit per key Q-limb is required");
    if (nPk != 0 && nPk != 1) return fail(HE_EINVAL, "he_evk_create_base2: a base-2 gadget takes at most one special prime");
    int beta = 0;
    for (int i = 0; i < n_rns; i++) {
        if (nj[i] <= 0 || nj[i] * pw2 > 64 + pw2) return fail(HE_EINVAL, "he_evk_create_base2: bad window count");
        beta += nj[i];
    }
    if (beta > 255) return fail(HE_EINVAL, "he_evk_create_base2: more than 255 gadget blocks");
    return evk_create_common(hev, beta, nQk, nPk, q, p, pw2, nj, n_rns, out);
}
int he_evk_destroy(he_handle h) { return unreg(h, T_EVK); }

int he_evk_device_buffer(he_handle hk, void **ptr, size_t *bytes) {
    GET(k, Evk, hk, T_EVK);
    if (!ptr || !bytes) return fail(HE_EINVAL, "he_evk_device_buffer: null output");
    Scope sc(k->ev->be->ctx.get());
    HIP_TRY(hipStreamSynchronize(k->ev->be->ctx->stream));  // the caller reads / writes it on a stream of its own
    *ptr = k->d;
    *bytes = (size_t)k->beta * 2 * (size_t)(k->nQk + k->nPk) * k->ev->be->Q->N * 8;
    return HE_OK;
}

int he_evk_download(he_handle hk, uint64_t *dst, size_t n_words) {
    GET(k, Evk, hk, T_EVK);
    const size_t words = (size_t)k->beta * 2 * (size_t)(k->nQk + k->nPk) * k->ev->be->Q->N;
    if (!dst || n_words != words) return fail(HE_EINVAL, "he_evk_download: the key holds %zu words", words);
    Scope sc(k->ev->be->ctx.get());
    HIP_TRY(hipStreamSynchronize(k->ev->be->ctx->stream));
    HIP_TRY(hipMemcpy(dst, k->d, words * 8, hipMemcpyDeviceToHost));
    return HE_OK;
}

int he_evk_commit(he_handle hk) {
    GET(k, Evk, hk, T_EVK);
    Scope sc(k->ev->be->ctx.get());
    if (int rc = evk_derive(*k)) return rc;
    HIP_TRY(hipStreamSynchronize(k->ev->be->ctx->stream));
    k->word_mul = 1;  // (an external writer supplies canonical words, as he_evk_create's caller does)
    return HE_OK;
}

namespace {
// BaseRNSDecompositionVectorSize, core/rlwe/params.go:543-550
int base_rns_size(int levelQ, int levelP) { return levelP == -1 ? levelQ + 1 : (levelQ + levelP + 1) / (levelP + 1); }
// digits of a gadget product with key k at levelQ (a base-2 gadget: the bit windows of limbs 0..levelQ)
int key_beta(const Evk &k, int levelQ) { return k.pw2 ? k.prefix[levelQ + 1] : base_rns_size(levelQ, k.nPk - 1); }

// The limbs of a QP element at (levelQ, levelP) in the order every launch table lists them: Q limbs 0..levelQ, then P limbs
// 0..levelP.  idx: the limb within its ring; mod: its row of the extender's constant tables.  cls: 0 every limb, 1 those NOT
// of the double-precision class (class 2), 2 that class only.  Q limbs [own0, own1) -- a digit's own -- are left out.
struct QPLimb {
    uint8_t idx, mod;
    bool isP;
};
int qp_limbs(const BasisExtender &be, int levelQ, int levelP, int cls, QPLimb *out, int own0 = 0, int own1 = 0) {
    int n = 0;
    for (int j = 0; j <= levelQ + levelP + 1; j++) {
        const bool isP = j > levelQ;
        const int idx = isP ? j - levelQ - 1 : j, mod = isP ? be.LQ + idx : idx;
        if (!isP && j >= own0 && j < own1) continue;
        if (cls && (be.small[mod] == 2) != (cls == 2)) continue;
        out[n++] = QPLimb{(uint8_t)idx, (uint8_t)mod, isP};
    }
    return n;
}
// ... as the limb tables of the two key inner products (KsArgs, NttMacArgs): digit limb, key limb, output limb and view
extern "C++" template <class A>
void key_product_limbs(A &a, const BasisExtender &be, const Evk &k, int levelQ, int levelP, int cls) {
    QPLimb l[kMaxLimbs];
    a.nlimbs = qp_limbs(be, levelQ, levelP, cls, l);
    for (int n = 0; n < a.nlimbs; n++) {
        a.dec_limb[n] = l[n].mod; a.key_limb[n] = (uint8_t)(l[n].isP ? k.nQk + l[n].idx : l[n].idx); a.out_limb[n] = l[n].idx;
        a.out_view[n] = l[n].isP ? 1 : 0; a.mod[n] = l[n].mod;
    }
}
// g^-1 mod 2N of an odd Galois element: the index the scattering stores use (NttEpilogue::scatter_ginv, KsScatter::ginv)
uint32_t galois_inverse(uint64_t gal, int logN) {
    const uint64_t mask = (2ull << logN) - 1;
    uint64_t x = gal & mask;
    for (int i = 0; i < 6; i++) x = (x * (2 - gal * x)) & mask;  // Newton
    return (uint32_t)x;
}

// DecomposeAndSplit for one digit (ring/basis_extension.go:381-502): coefficient-domain src
// (limbs of ringQ) -> dstQ limbs (dstQ_limb0 + j) and dstP limbs (dstP_limb0 + j).
// own_too: for single-limb digits the reference also rewrites the digit's own limb.
int decompose_digit(Evaluator &ev, int levelQ, int levelP, int nbPi, int digit, View src, View dstQ, int dstQ_limb0, View dstP,
                    int dstP_limb0, int batch) {
    BasisExtender &be = *ev.be;
    const int st = digit * nbPi;
    int ed = st + nbPi;
    if (ed > levelQ + 1) ed = levelQ + 1;
    if (st > levelQ) return fail(HE_EINVAL, "DecomposeAndSplit: digit %d out of range at levelQ %d", digit, levelQ);
    int decompLvl;
    if (levelQ > nbPi * (digit + 1) - 1) decompLvl = nbPi - 2;
    else decompLvl = (levelQ % nbPi) - 1;
    ModUpArgs a{};
    const bool single = decompLvl < 0;
    std::vector<uint64_t> basis(be.Q->moduli.begin() + st, be.Q->moduli.begin() + ed);
    QPLimb l[kMaxLimbs];
    a.ndst = qp_limbs(be, levelQ, levelP, 0, l, single ? 0 : st, single ? 0 : ed);
    for (int n = 0; n < a.ndst; n++) {
        a.dst_limb[n] = (uint8_t)((l[n].isP ? dstP_limb0 : dstQ_limb0) + l[n].idx); a.dst_mod[n] = a.dst_row[n] = l[n].mod;
        a.dst_view[n] = l[n].isP ? 1 : 0;
        a.dst_half[n] = single ? 0 : half_product_mod(basis, be.modulus(l[n].mod));
    }
    if (single) {
        a.nsrc = 1; a.src_limb[0] = (uint8_t)st; a.src_mod[0] = (uint8_t)st;
        HIP_TRY(launch_center_copy(be.qp, a, src, dstQ, dstP, batch, be.ctx->stream));
        return HE_OK;
    }
    if (nbPi < 2 || nbPi - 2 >= (int)ev.dec.size() || digit >= (int)ev.dec[nbPi - 2].size() || decompLvl >= (int)ev.dec[nbPi - 2][digit].size())
        return fail(HE_EINVAL, "DecomposeAndSplit: no constants for nbPi=%d digit=%d", nbPi, digit);
    const ModUpRef &ref = ev.dec[nbPi - 2][digit][decompLvl];
    a.nsrc = ed - st;
    for (int i = 0; i < a.nsrc; i++) {
        a.src_limb[i] = (uint8_t)(st + i); a.src_mod[i] = (uint8_t)(st + i);
        a.src_half[i] = half_product_mod(basis, be.Q->moduli[st + i]);
    }
    HIP_TRY(launch_modup(be.qp, ref.on(ev.pool), a, src, dstQ, dstP, batch, be.ctx->stream));
    return HE_OK;
}

// DecomposeNTT (core/rlwe/evaluator_gadget_product.go:459-510) into a Decomp buffer.
// c2ntt / c2inv: NTT-domain and coefficient-domain views of the input (levelQ+1 limbs).
int decompose_ntt_into(Evaluator &ev, int levelQ, int levelP, int nbPi, View c2ntt, View c2inv, View dec, size_t dec_ds, int batch) {
    BasisExtender &be = *ev.be;
    const int LQ = be.LQ;
    const int beta = base_rns_size(levelQ, levelP);
    hipStream_t st = be.ctx->stream;
    if (dec_ds != (size_t)(be.LQ + be.LP) * be.Q->N) return fail(HE_EINVAL, "decompose: unexpected digit stride");
    for (int d = 0; d < beta; d++) {
        View blk{dec.p + (size_t)d * dec_ds, dec.bstride, dec.tab};
        TRY(decompose_digit(ev, levelQ, levelP, nbPi, d, c2inv, blk, 0, blk, LQ, batch));
        const int s0 = d * nbPi, e0 = std::min(s0 + nbPi, levelQ + 1);
        LimbTab t;  // NTT of every limb except the digit's own
        QPLimb l[kMaxLimbs];
        t.n = qp_limbs(be, levelQ, levelP, 0, l, s0, e0);
        for (int i = 0; i < t.n; i++) t.in_limb[i] = t.out_limb[i] = t.mod[i] = l[i].mod;
        const bool red = modup_out_needs_reduce(std::vector<uint64_t>(be.Q->moduli.begin() + s0, be.Q->moduli.begin() + e0));
        HIP_TRY(be_ntt(be, t, blk, blk, batch, false, red ? NTT_REDUCE_INPUT : 0));
        // own limbs: copy of the NTT-domain input                         evaluator_gadget_product.go:498-503
        HIP_TRY(launch_ew(be.qp, ident_tab(e0 - s0, s0, s0, s0), EW_COPY, c2ntt, c2ntt, blk, batch, nullptr, nullptr, st));
    }
    return HE_OK;
}

// inner product of a decomposition with a key (gadgetProductMultiplePLazyHoisted :401-453)
// limb_filter: 0 = every limb, 1 = only limbs NOT of class 2 (the fused f64 NTT+MAC kernel takes the others)
int ks_inner(Evaluator &ev, int levelQ, int levelP, View dec, size_t dec_ds, const Evk &k, View o0Q,
             View o0P, View o1Q, View o1P, int batch, const View *own = nullptr, int own_alpha = 0, int limb_filter = 0,
             int digit_begin = 0, int digit_end = -1, const KsScatter *scatter = nullptr) {
    BasisExtender &be = *ev.be;
    const int N = be.Q->N;
    KsArgs a{};
    a.beta = key_beta(k, levelQ);
    if (a.beta > k.beta) return fail(HE_EINVAL, "gadget product: key has %d digits, %d needed", k.beta, a.beta);
    const uint64_t *keyp = k.d;
    if (digit_end >= 0) {  // a sub-range of the digits (he_gadget_product_hoisted_lazy_digits): shift both operands
        if (own || digit_begin < 0 || digit_end > a.beta || digit_begin >= digit_end) return fail(HE_EINVAL, "gadget product: bad digit range");
        dec.p += (size_t)digit_begin * dec_ds;
        keyp += (size_t)digit_begin * 2 * (size_t)(k.nQk + k.nPk) * N;
        a.beta = digit_end - digit_begin;
    }
    key_product_limbs(a, be, k, levelQ, levelP, limb_filter);
    const int n = a.nlimbs;
    a.dec_dstride = dec_ds;
    a.key_kstride = (size_t)(k.nQk + k.nPk) * N;
    a.key_dstride = 2 * a.key_kstride;
    a.own_alpha = own ? own_alpha : 0;
    a.own_nq = levelQ + 1;
    const View decv = dec;
    if (scatter && scatter->ginv) {  // (add_s arrives by Q limb: compact it to the launch limbs)
        KsScatter sc = *scatter;
        for (int i = 0; i < n; i++) sc.add_s[i] = (a.out_view[i] == 0 && !scatter->plain) ? scatter->add_s[a.out_limb[i]] : 0;
        HIP_TRY(launch_ks_inner(be.qp, a, decv, own ? *own : decv, keyp, o0Q, o0P, o1Q, o1P, batch, be.ctx->stream, &sc));
        return HE_OK;
    }
    HIP_TRY(launch_ks_inner(be.qp, a, decv, own ? *own : decv, keyp, o0Q, o0P, o1Q, o1P, batch, be.ctx->stream));
    return HE_OK;
}

// ---- fused pipeline plans ------------------------------------------------------------------
// which destinations of a descriptor take the lean integer path of modup_fused_kernel (see there): moduli below 2^58 that are
// not on the double-precision path, column sums that cannot overflow, and a sum that one Montgomery reduction brings below 2p
void mark_fast_destinations(const BasisExtender &be, ModUpDesc &D, const std::vector<uint64_t> &basis) {
    static const bool off = env_flag("HERING_NO_FAST_MODUP");
    uint64_t mx = 0;
    for (uint64_t m : basis) mx = std::max(mx, m);
    for (int j = 0; j < D.ndst; j++) {
        const uint64_t p = be.modulus(D.dst_mod[j]);
        const bool f64_dst = (p >> 47) == 0 && be.d_twdf != nullptr;
        const u128 colsum = (u128)(D.nsrc + 1) * ((u128)p + mx + ((u128)1 << 31));
        // radix-2^30 reduction of the lean sum (HE_MODUP_R60): the middle column takes (nsrc + 1) (x1 t0 + x0 t1) + m0 p1 + a carry + m1 p0,
        // and the result (sum + m p) / 2^60 stays below 2p only while (nsrc + 1) max q <= 2^60
        const u128 midcol = (u128)(D.nsrc + 1) * ((((u128)(mx >> 30) + 1) << 30) + (((u128)(p >> 30) + 1) << 30)) +
                            (((u128)(p >> 30) + 1) << 30) + ((u128)1 << 35) + ((u128)1 << 60);  // ... + m0 p1 + carry + m1 p0
        const bool r60 = (midcol >> 64) == 0 && (u128)(D.nsrc + 1) * mx <= ((u128)1 << 60) && D.nsrc + 2 <= 15;
        // 1: 30-bit column accumulation + correction-free butterflies (below 2^58); 2: 128-bit accumulation + Harvey-range
        // butterflies (any modulus); 0: the generic path (single-limb digits, sums that need the extra reduction)
        const bool lean = !off && !D.single && !D.reduce_out && !f64_dst && be.d_tws != nullptr;
        D.dst_fast[j] = !lean ? 0 : ((p >> 58) == 0 && D.nsrc + 1 <= 15 && (colsum >> 64) == 0) ? (HE_MODUP_R60 && r60 ? 3 : 1) : 2;
    }
}
// the constants of one basis extension, as a fused descriptor holds them
void desc_constants(ModUpDesc &D, const ModUpRef &ref, const ConstPool &pool, const std::vector<uint64_t> &basis) {
    const ModUpDev c = ref.on(pool);
    D.a = c.a; D.T = c.T; D.vt = c.vt;
    D.Td = ref.Td_on(pool); D.vtd = ref.vtd_on(pool);
    D.fc = ref.fc_on(pool); D.t60 = ref.t60_on(pool);
    D.reduce_out = modup_out_needs_reduce(basis) ? 1 : 0;
}
int upload_plan(Evaluator &ev, const std::vector<ModUpDesc> &descs, FusedPlan &plan) {
    plan.ok = !descs.empty();
    for (const ModUpDesc &d : descs)
        if (!modup_fused_supported(ev.be->Q->logN, d.nsrc)) plan.ok = false;
    if (!plan.ok) return HE_OK;
    ModUpDesc *dev = nullptr;
    HIP_TRY(hipMalloc((void **)&dev, descs.size() * sizeof(ModUpDesc)));
    HIP_TRY(hipMemcpy(dev, descs.data(), descs.size() * sizeof(ModUpDesc), hipMemcpyHostToDevice));
    ev.plan_mem.push_back(dev);
    size_t i = 0;
    while (i < descs.size()) {
        size_t j = i;
        while (j < descs.size() && descs[j].nsrc == descs[i].nsrc) j++;
        int cls = 0;
        for (size_t k = i; k < j; k++)
            for (int t = 0; t < descs[k].ndst; t++) cls |= (ev.be->modulus(descs[k].dst_mod[t]) >> 47) ? 1 : 2;
        int limbs = 0;
        for (size_t k = i; k < j; k++) limbs += descs[k].nsrc + descs[k].ndst;
        plan.groups.push_back(FusedGroup{dev + i, (int)(j - i), descs[i].nsrc, cls, limbs});
        i = j;
    }
    return HE_OK;
}
// all digits of DecomposeNTT at (levelQ, levelP, nbPi) into a [beta][LQ+LP][N] block per batch entry
int get_dec_plan(Evaluator &ev, int levelQ, int levelP, int nbPi, const FusedPlan **out) {
    auto key = std::make_tuple(levelQ, levelP, nbPi);
    auto it = ev.dec_plans.find(key);
    if (it != ev.dec_plans.end()) { *out = &it->second; return HE_OK; }
    BasisExtender &be = *ev.be;
    const int width = be.LQ + be.LP, N = be.Q->N;
    const int beta = base_rns_size(levelQ, levelP);
    std::vector<ModUpDesc> descs;
    bool ok = true;
    for (int d = 0; d < beta && ok; d++) {
        const int st = d * nbPi, ed = std::min(st + nbPi, levelQ + 1);
        if (st > levelQ) { ok = false; break; }
        int decompLvl = (levelQ > nbPi * (d + 1) - 1) ? nbPi - 2 : (levelQ % nbPi) - 1;
        ModUpDesc D;
        memset(&D, 0, sizeof D);
        D.single = decompLvl < 0;
        D.nsrc = ed - st;
        if (D.nsrc > 8) { ok = false; break; }
        std::vector<uint64_t> basis(be.Q->moduli.begin() + st, be.Q->moduli.begin() + ed);
        if (!D.single) {
            if (nbPi < 2 || nbPi - 2 >= (int)ev.dec.size() || d >= (int)ev.dec[nbPi - 2].size() ||
                decompLvl >= (int)ev.dec[nbPi - 2][d].size()) { ok = false; break; }
            const ModUpRef &ref = ev.dec[nbPi - 2][d][decompLvl];
            desc_constants(D, ref, ev.pool, basis);
        }
        for (int i = 0; i < D.nsrc; i++) {
            D.src_limb[i] = (uint8_t)(st + i); D.src_mod[i] = (uint8_t)(st + i);
            D.src_half[i] = D.single ? 0 : half_product_mod(basis, be.Q->moduli[st + i]);
            D.src_split[i] = (be.Q->moduli[st + i] >> 51) ? 1 : 0;
        }
        D.dst_off = (size_t)d * width * N;
        QPLimb l[kMaxLimbs];
        D.ndst = qp_limbs(be, levelQ, levelP, 0, l, st, ed);  // own limbs come from the NTT-domain input
        for (int n = 0; n < D.ndst; n++) {
            D.dst_limb[n] = D.dst_mod[n] = D.dst_row[n] = l[n].mod; D.dst_view[n] = 0;
            D.dst_half[n] = D.single ? 0 : half_product_mod(basis, be.modulus(l[n].mod));
        }
        mark_fast_destinations(be, D, basis);
        descs.push_back(D);
    }
    FusedPlan plan;
    // (conjugate-invariant rings: the fold sits between the inverse network and the basis extension, and it pairs coefficient j
    // with N - j -- not thread-local in the fused kernel; those rings take the unfused launches)
    if (ok && beta * width <= 256 && be.type == 0) TRY(upload_plan(ev, descs, plan));
    auto ins = ev.dec_plans.emplace(key, plan);
    *out = &ins.first->second;
    return HE_OK;
}
// ModUpPtoQ inside ModDownQPtoQNTT at (levelQ, levelP)
int get_md_plan(Evaluator &ev, int levelQ, int levelP, const FusedPlan **out) {
    auto key = std::make_pair(levelQ, levelP);
    auto it = ev.md_plans.find(key);
    if (it != ev.md_plans.end()) { *out = &it->second; return HE_OK; }
    BasisExtender &be = *ev.be;
    std::vector<uint64_t> basis;
    if (levelP >= 0) basis.assign(be.P->moduli.begin(), be.P->moduli.begin() + levelP + 1);
    ModUpDesc D;
    memset(&D, 0, sizeof D);
    D.nsrc = levelP + 1;
    FusedPlan plan;
    if (levelP >= 0 && D.nsrc <= 8 && be.type == 0) {  // levelP = -1 (no special primes): ModDown is a copy, no plan (plan.ok stays false)
        desc_constants(D, be.ptoq[levelP], be.pool, basis);
        for (int i = 0; i <= levelP; i++) {
            D.src_limb[i] = (uint8_t)i; D.src_mod[i] = (uint8_t)(be.LQ + i);
            D.src_half[i] = half_product_mod(basis, be.P->moduli[i]);
            D.src_split[i] = (be.P->moduli[i] >> 51) ? 1 : 0;
        }
        for (int j = 0; j <= levelQ; j++) {
            D.dst_limb[j] = (uint8_t)j; D.dst_mod[j] = (uint8_t)j; D.dst_row[j] = (uint8_t)j; D.dst_view[j] = 0;
            D.dst_half[j] = half_product_mod(basis, be.Q->moduli[j]);
        }
        D.ndst = levelQ + 1;
        mark_fast_destinations(be, D, basis);
        TRY(upload_plan(ev, std::vector<ModUpDesc>{D}, plan));
    }
    auto ins = ev.md_plans.emplace(key, plan);
    *out = &ins.first->second;
    return HE_OK;
}
// forward ROWS pass over every non-own limb of every digit block of a decomposition
// limb_filter 1: skip the class-2 limbs (their transform is fused into launch_ntt_mac_f64)
int dec_rows_ntt(Evaluator &ev, int levelQ, int levelP, int nbPi, View dec, int batch, int limb_filter = 0) {
    BasisExtender &be = *ev.be;
    const int width = be.LQ + be.LP;
    const int beta = base_rns_size(levelQ, levelP);
    LimbTab t;
    t.n = 0;
    auto flush = [&]() -> int {
        if (t.n == 0) return HE_OK;
        HIP_TRY(launch_ntt_rows(be.qp, t, dec, dec, batch, false, 0, be.ctx->stream));
        t.n = 0;
        return HE_OK;
    };
    for (int d = 0; d < beta; d++) {
        QPLimb l[kMaxLimbs];
        const int n = qp_limbs(be, levelQ, levelP, limb_filter, l, d * nbPi, std::min(d * nbPi + nbPi, levelQ + 1));
        for (int i = 0; i < n; i++) {
            t.in_limb[t.n] = t.out_limb[t.n] = (uint8_t)(d * width + l[i].mod);
            t.mod[t.n] = l[i].mod;
            if (++t.n == kMaxLimbs) TRY(flush());
        }
    }
    return flush();
}

// scratch of a gadget product over `batch` entries: inverse transform and digits (need_dec), the accumulators, as much for ModDown
size_t ks_scratch_words(const BasisExtender &be, int levelQ, int levelP, int batch, bool need_dec, const Evk *key = nullptr) {
    const size_t N = be.Q->N, B = batch;
    const size_t beta = key ? (size_t)key_beta(*key, levelQ) : (size_t)base_rns_size(levelQ, levelP);
    size_t w = 0;
    if (need_dec) w += B * (levelQ + 1) * N + B * beta * (be.LQ + be.LP) * N;
    w += 2 * B * (levelP + 1) * N * 2 + 2 * B * (levelQ + 1) * N * 2;
    return w + 64;
}
// The scratch each of these entries' launches reserve and take, as the entry itself and a call composed of several of them
// (he_lintrans_evaluate_many) size it: ONE expression per step.
size_t decompose_ntt_words(const BasisExtender &be, int levelQ, int B) { return (size_t)B * (levelQ + 1) * be.Q->N; }
size_t auto_hoisted_lazy_words(const BasisExtender &be, int levelQ, int levelP, int B) {
    const size_t N = be.Q->N;
    return 3 * (size_t)B * (levelQ + 1) * N + 2 * (size_t)B * (levelP + 1) * N + N + 64;
}
size_t giant_step_words(const BasisExtender &be, int levelQ, int levelP, int B, const Evk *k) {
    return ks_scratch_words(be, levelQ, levelP, B, true, k) + 2 * (size_t)B * (levelQ + levelP + 2) * be.Q->N + 64;
}
size_t eval_moddown_words(const BasisExtender &be, int levelQ, int levelP, int B) { return (size_t)B * (levelQ + levelP + 2) * be.Q->N; }
}  // namespace

namespace {
int decompose_fused(Evaluator &ev, const FusedPlan &plan, int levelQ, int levelP, int nbPi, View rows_inv, View dec, int batch,
                    int ntt_filter = 0, bool f64_raw = false);
}
static int decompose_ntt_run(const std::shared_ptr<Evaluator> &ev, int levelQ, int levelP, int nbPi, int c2_is_ntt, size_t dec_ds,
                             const View *v, int B);
int he_decompose_and_split(he_handle hev, int levelQ, int levelP, int nbPi, int digit, he_handle h0, he_handle h1q, he_handle h1p) {
    GET(ev, Evaluator, hev, T_EVAL);
    BasisExtender &be = *ev->be;
    if (levelQ < 0 || levelQ >= be.LQ || levelP < 0 || levelP >= be.LP || nbPi < 1 || digit < 0)
        return fail(HE_EINVAL, "he_decompose_and_split: bad level/digit");
    CoReq q;
    Operands o(q, "he_decompose_and_split", be);
    o.in(h0, levelQ + 1);
    o.out(h1q, levelQ + 1);
    o.outP(h1p, levelP + 1);
    TRY(o.check());
    q.op = CO_DECOMPOSE_SPLIT; q.obj = ev.get(); q.par[0] = levelQ; q.par[1] = levelP; q.par[2] = nbPi; q.par[3] = digit;
    q.keep.push_back(ev);
    q.run = [ev, levelQ, levelP, nbPi, digit](const View *v, int B) -> int {
        BasisExtender &be = *ev->be;
        be.ctx->acct(std::min(nbPi, levelQ + 1 - digit * nbPi) + levelQ + 1 + levelP + 1, 0, B, be.Q->N);  // ModUp of one digit
        {
            Valu V(be.Q->logN);
            const int s0 = digit * nbPi, e0 = std::min(s0 + nbPi, levelQ + 1);
            std::vector<int> d;
            for (int i = 0; i <= levelQ; i++) if (i < s0 || i >= e0) d.push_back(i);
            for (int j = 0; j <= levelP; j++) d.push_back(be.LQ + j);
            valu_modup(V, be.small, s0, e0 - s0, d);
            V.into(*be.ctx, B);
        }
        return decompose_digit(*ev, levelQ, levelP, nbPi, digit, v[0], v[1], 0, v[2], 0, B);
    };
    return co_dispatch(*be.ctx, o.B, q);
}

int he_decomp_create(he_handle hev, int batch, he_handle *out) {
    GET(ev, Evaluator, hev, T_EVAL);
    if (batch <= 0 || !out) return fail(HE_EINVAL, "he_decomp_create: bad batch");
    BasisExtender &be = *ev->be;
    if (be.LP == 0) return fail(HE_EINVAL, "he_decomp_create: hoisted decompositions need special primes (the reference's DecomposeNTT dereferences ringP)");
    auto d = std::make_shared<Decomp>();
    d->ev = ev;
    d->batch = batch;
    d->beta_max = base_rns_size(be.LQ - 1, be.LP - 1);  // digits at (max levelQ, max levelP)
    d->width = be.LQ + be.LP;
    // (no stream work here: the buffer cache has its own lock -- a caller that creates a hoisting buffer neither waits for the
    // context nor, in deferred mode, for its own pending requests)
    HIP_TRY(hipSetDevice(be.ctx->dev));
    const size_t bytes = (size_t)batch * d->bstride() * 8;
    hipError_t e = be.ctx->pool_take(bytes, (void **)&d->d);
    if (e != hipSuccess) {
        d->d = nullptr;
        return fail(HE_ENOMEM, "he_decomp_create: hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    }
    *out = reg(d);
    return HE_OK;
}
int he_decomp_destroy(he_handle h) { return unreg(h, T_DECOMP); }
int he_decomp_download_limb(he_handle h, int b, int digit, int is_p, int limb, uint64_t *dst) {
    GET(d, Decomp, h, T_DECOMP);
    BasisExtender &be = *d->ev->be;
    if (!dst || b < 0 || b >= d->batch || digit < 0 || digit >= d->beta_max || limb < 0 || limb >= (is_p ? be.LP : be.LQ))
        return fail(HE_EINVAL, "he_decomp_download_limb: bad index");
    Scope sc(be.ctx.get());
    const uint64_t *src = d->d + (size_t)b * d->bstride() + (size_t)digit * d->dstride() + (size_t)((is_p ? be.LQ : 0) + limb) * be.Q->N;
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)be.Q->N * 8, hipMemcpyDeviceToHost, be.ctx->stream));
    HIP_TRY(hipStreamSynchronize(be.ctx->stream));
    return HE_OK;
}

int he_decompose_ntt(he_handle hev, int levelQ, int levelP, int nbPi, he_handle hc2, int c2_is_ntt, he_handle hdec) {
    GET(ev, Evaluator, hev, T_EVAL);
    GET(dec, Decomp, hdec, T_DECOMP);
    BasisExtender &be = *ev->be;
    if (dec->ev != ev) return fail(HE_EINVAL, "he_decompose_ntt: decomposition buffer belongs to another evaluator");
    if (levelQ < 0 || levelQ >= be.LQ || levelP < 0 || levelP >= be.LP) return fail(HE_EINVAL, "he_decompose_ntt: level out of range");
    if (base_rns_size(levelQ, levelP) > dec->beta_max) return fail(HE_EINVAL, "he_decompose_ntt: too many digits");
    CoReq q;
    Operands o(q, "he_decompose_ntt", be, dec->batch);
    o.in(hc2, levelQ + 1);
    o.raw(dec->view(), dec);
    TRY(o.check());
    dec->fillQ = -1;  // not filled until every launch below has been enqueued (check_decomp refuses a partial buffer)
    const size_t dec_ds = dec->dstride();
    q.op = CO_DECOMPOSE_NTT; q.obj = ev.get(); q.par[0] = levelQ; q.par[1] = levelP; q.par[2] = nbPi; q.par[3] = c2_is_ntt;
    q.keep.push_back(ev);
    q.run = [ev, levelQ, levelP, nbPi, c2_is_ntt, dec_ds](const View *v, int B) -> int {
        return decompose_ntt_run(ev, levelQ, levelP, nbPi, c2_is_ntt, dec_ds, v, B);
    };
    q.tables_ok = [ev](bool *ok) -> int { *ok = ev->be->type == 0; return HE_OK; };
    TRY(co_dispatch(*be.ctx, o.B, q));
    dec->fillQ = levelQ; dec->fillP = levelP; dec->fill_beta = base_rns_size(levelQ, levelP);
    return HE_OK;
}
// the launches of DecomposeNTT over B entries: v = (c2, the hoisting buffer [B][digits][LQ + LP][N] with digit stride dec_ds).
// The caller holds the context (Scope).
static int decompose_ntt_run(const std::shared_ptr<Evaluator> &ev, int levelQ, int levelP, int nbPi, int c2_is_ntt, size_t dec_ds,
                             const View *v, int B) {
    BasisExtender &be = *ev->be;
    const int N = be.Q->N;
    be.ctx->acct(levelQ + 1 + (double)base_rns_size(levelQ, levelP) * (levelQ + levelP + 2), 0, B, N);  // DecomposeNTT: L in, beta (L + alpha) out
    { Valu V(be.Q->logN); valu_keyswitch(V, be, levelQ, levelP, base_rns_size(levelQ, levelP), true, false); V.into(*be.ctx, B); }
    const size_t w = decompose_ntt_words(be, levelQ, B);
    TRY(be.ctx->arena_reserve(w));
    View other{be.ctx->arena_take(w), (size_t)(levelQ + 1) * N};
    View ntt = v[0], inv = other;
    if (c2_is_ntt) {
        const FusedPlan *plan = nullptr;
        TRY(get_dec_plan(*ev, levelQ, levelP, nbPi, &plan));
        if (plan->ok) {
            HIP_TRY(launch_ntt_rows(be.qp, ident_tab(levelQ + 1), v[0], other, B, true, NTT_REDUCE_INPUT, be.ctx->stream));
            TRY(decompose_fused(*ev, *plan, levelQ, levelP, nbPi, other, v[1], B));
            const int beta = base_rns_size(levelQ, levelP);
            for (int d = 0; d < beta; d++) {  // own limbs: copy of the NTT-domain input (evaluator_gadget_product.go:498-503)
                const int s0 = d * nbPi, e0 = std::min(s0 + nbPi, levelQ + 1);
                View blk{v[1].p + (size_t)d * dec_ds, v[1].bstride, v[1].tab};
                HIP_TRY(launch_ew(be.qp, ident_tab(e0 - s0, s0, s0, s0), EW_COPY, v[0], v[0], blk, B, nullptr, nullptr, be.ctx->stream));
            }
            return HE_OK;
        }
        HIP_TRY(be_ntt(be, ident_tab(levelQ + 1), v[0], other, B, true, NTT_REDUCE_INPUT));
    } else {
        HIP_TRY(be_ntt(be, ident_tab(levelQ + 1), v[0], other, B, false, NTT_REDUCE_INPUT));
        ntt = other; inv = v[0];
    }
    return decompose_ntt_into(*ev, levelQ, levelP, nbPi, ntt, inv, v[1], dec_ds, B);
}

namespace {
// DecomposeNTT through the fused kernels: `rows_inv` = inverse ROWS pass of the NTT-domain input.
// Own limbs are NOT written (ks_inner reads them from the input; he_decompose_ntt copies them).
int decompose_fused(Evaluator &ev, const FusedPlan &plan, int levelQ, int levelP, int nbPi, View rows_inv, View dec, int batch,
                    int ntt_filter, bool f64_raw) {
    BasisExtender &be = *ev.be;
    const View dv = dec;
    for (const FusedGroup &g : plan.groups)
        HIP_TRY(launch_modup_fused(be.qp, g.dev, g.n, g.nsrc, g.dst_classes, rows_inv, dv, dv, batch, be.ctx->stream, f64_raw, g.total_limbs));
    return dec_rows_ntt(ev, levelQ, levelP, nbPi, dec, batch, ntt_filter);
}
// May the basis extension hand unreduced doubles to the double-precision row kernels (launch_modup_fused f64_raw)?
static bool f64_raw_ok(const BasisExtender &be, int levelQ, int levelP, int nsrc) {
    uint64_t mx = 0;
    for (int j = 0; j <= levelQ; j++) if (be.small[j] == 2) mx = std::max(mx, be.Q->moduli[j]);
    for (int j = 0; j <= levelP; j++) if (be.small[be.LQ + j] == 2) mx = std::max(mx, be.P->moduli[j]);
    return mx != 0 && modup_f64_raw_ok(be.Q->logN, nsrc, mx);
}
// The digits the NTT + MAC kernel reads (raw: the double-precision limbs as unreduced doubles).  With the MAC epilogue the lazy
// core leaves that launch pending: gadget_product_core runs it after the extension of the P part, the ModDown epilogue inside.
struct MacDigits {
    const uint64_t *dec = nullptr;
    size_t bs = 0, ds = 0;
    bool raw = false, own_reduce = true;
};
// the four inputs of a ciphertext product whose c0 / c1 the fused ModDown epilogue forms itself (NttEpilogue::tensor).  The
// operand of such a key switch is the (not yet computed) degree-2 term T(a1, b1): gadget_product_lazy_core forms it -- in the
// inverse row pass itself for the limbs of the double-precision class where the route has the prologue (NttProdIn), by
// launch_tensor otherwise
struct TensorIn {
    View a0, a1, b0, b1;
    const uint64_t *ts;  // per Q limb
};
// what a lazy gadget product runs on: cx (NTT domain) -> accumulators (views); scratch from the arena
struct LazyArgs {
    View cx;
    int B = 0;
    View c0Q, c0P, c1Q, c1P;          // the four accumulators (null P views: no special primes)
    bool cx_canonical = false;        // cx was produced by this library and is known to be in [0, q) (no input reduction)
    const TensorIn *tin = nullptr;    // with route.tensor_epilogue
    const KsScatter *giant = nullptr; // with route.giant_fused: the accumulators leave through KsScatter's giant-step stores
    MacDigits *pending = nullptr;     // with route.moddown == KS_MD_FUSED_MAC: the launch that is left to the caller
};
// class-2 limbs of the gadget product (m.cx, the accumulators, m.B, m.giant): forward row NTT + key MAC in one kernel
// epi (optional): the ModDown epilogue runs in the kernel (NttMacEpilogue; sp / tsp indexed by Q LIMB here, compacted below)
int ks_mac_f64(Evaluator &ev, int levelQ, const Evk &k, const KsRoute &r, const LazyArgs &m, const MacDigits &dec, const NttMacEpilogue *epi) {
    BasisExtender &be = *ev.be;
    const hipStream_t st = be.ctx->stream;
    const int levelP = k.nPk - 1, N = be.Q->N;
    NttMacArgs a{};
    a.beta = base_rns_size(levelQ, levelP);
    key_product_limbs(a, be, k, levelQ, levelP, 2);
    a.dec_dstride = dec.ds;
    a.key_kstride = (size_t)(k.nQk + k.nPk) * N;
    a.key_dstride = 2 * a.key_kstride;
    a.own_alpha = levelP + 1;
    a.own_nq = levelQ + 1;
    a.own_reduce = dec.own_reduce ? 1 : 0;
    a.dec_f64 = dec.raw ? 1 : 0;
    a.q_out_f64 = 0;
    const View decv{const_cast<uint64_t *>(dec.dec), dec.bs};
    if (epi) {
        NttMacEpilogue e = *epi;
        for (int i = 0; i < a.nlimbs; i++) { e.sp[i] = epi->sp[a.out_limb[i]]; e.tsp[i] = epi->tsp[a.out_limb[i]]; }
        HIP_TRY(launch_ntt_mac_f64(be.qp, a, decv, m.cx, k.keyd, m.c0Q, m.c0P, m.c1Q, m.c1P, m.B, st, &e));
        return HE_OK;
    }
    if (!r.acc_q_f64) {
        HIP_TRY(launch_ntt_mac_f64(be.qp, a, decv, m.cx, k.keyd, m.c0Q, m.c0P, m.c1Q, m.c1P, m.B, st, nullptr, m.giant));
        return HE_OK;
    }
    // double-format Q accumulators: the Q limbs and the P limbs go to separate launches (different store code)
    NttMacArgs aq = a, ap = a;
    key_product_limbs(aq, be, k, levelQ, -1, 2);
    key_product_limbs(ap, be, k, -1, levelP, 2);
    aq.q_out_f64 = 1;
    HIP_TRY(launch_ntt_mac_f64(be.qp, aq, decv, m.cx, k.keyd, m.c0Q, m.c0P, m.c1Q, m.c1P, m.B, st));
    HIP_TRY(launch_ntt_mac_f64(be.qp, ap, decv, m.cx, k.keyd, m.c0Q, m.c0P, m.c1Q, m.c1P, m.B, st));
    return HE_OK;
}
// the route of one call with the two plans it was decided from (null: a base-2 gadget; no special primes)
struct KsCall {
    KsRoute route;
    const FusedPlan *dec = nullptr, *md = nullptr;
};
// windows of source limb i of a bit-window accumulation: the key's, or one per limb (BaseTwoDecomposition == 0 in core/rgsw)
int rgsw_nj(const Evk &k, int i) { return k.pw2 ? k.nj[i] : 1; }
// Bit-window accumulation of one polynomial against a key: windows (INTT(cx)[i] >> j pw2) & mask of every Q limb, NTT'd into every
// limb, multiplied into the accumulators (core/rlwe/evaluator_gadget_product.go:203-338; core/rgsw/evaluator.go:139-203 for one
// el).  pw2 == 0 is core/rgsw's all-ones mask, one uncentred window per limb (:147-149).  reduce_wide: windows that can reach the
// modulus they are transformed in are reduced first (core/rgsw's shapes; rlwe's base-2 keys never have them).
int window_products_core(Evaluator &ev, int levelQ, const Evk &k, const LazyArgs &a, bool reduce_wide) {
    BasisExtender &be = *ev.be;
    const int levelP = k.nPk - 1, N = be.Q->N, B = a.B;
    int beta = 0;
    for (int i = 0; i <= levelQ; i++) beta += rgsw_nj(k, i);
    const size_t wq = (size_t)B * (levelQ + 1) * N, ds = (size_t)(be.LQ + be.LP) * N, bs = (size_t)beta * ds;
    View inv{be.ctx->arena_take(wq), (size_t)(levelQ + 1) * N};
    uint64_t *dec = be.ctx->arena_take((size_t)B * bs);
    hipStream_t st = be.ctx->stream;
    HIP_TRY(be_ntt(be, ident_tab(levelQ + 1), a.cx, inv, B, true, NTT_REDUCE_INPUT));
    MaskSpreadArgs m{};
    m.mask = k.pw2 ? ((uint64_t)1 << k.pw2) - 1 : ~(uint64_t)0;
    LimbTab t;
    QPLimb l[kMaxLimbs];
    t.n = m.ndst = qp_limbs(be, levelQ, levelP, 0, l);
    bool reduce = false;
    for (int j = 0; j < t.n; j++) {
        t.in_limb[j] = t.out_limb[j] = t.mod[j] = m.dst_limb[j] = l[j].mod;
        reduce = reduce || (reduce_wide && m.mask >= be.modulus(l[j].mod));
    }
    for (int i = 0; i <= levelQ; i++)
        for (int j = 0; j < rgsw_nj(k, i); j++) {
            m.blk_limb[m.nblk] = (uint8_t)i;
            m.blk_shift[m.nblk] = (uint8_t)(j * k.pw2);  // <= 64 (he_evk_create_base2); 64: a window of zero
            m.nblk++;
        }
    HIP_TRY(launch_mask_spread(be.qp, m, inv, dec, bs, ds, B, st));
    for (int d = 0; d < beta; d++) {
        View blk{dec + (size_t)d * ds, bs};
        HIP_TRY(be_ntt(be, t, blk, blk, B, false, reduce ? NTT_REDUCE_INPUT : 0));
    }
    return ks_inner(ev, levelQ, levelP, View{dec, bs}, ds, k, a.c0Q, a.c0P, a.c1Q, a.c1P, B);
}
// GadgetProductLazy core: the digits of a.cx as the route makes them, multiplied into the accumulators
int gadget_product_lazy_core(Evaluator &ev, int levelQ, const Evk &k, const KsCall &c, const LazyArgs &a) {
    BasisExtender &be = *ev.be;
    const KsRoute &r = c.route;
    const int levelP = k.nPk - 1, N = be.Q->N, B = a.B;
    const int beta = key_beta(k, levelQ);
    const size_t wq = (size_t)B * (levelQ + 1) * N, ds = (size_t)(be.LQ + be.LP) * N, bs = (size_t)beta * ds;
    const View cx = a.cx;
    if (a.tin) {
        // cx = T(a1, b1): everywhere by the tensor kernel, or -- with the prologue -- only on the integer-class limbs, the others
        // being formed by the inverse row pass below
        LimbTab tt;
        QPLimb l[kMaxLimbs];
        uint64_t tsv[kMaxLimbs];
        tt.n = qp_limbs(be, levelQ, -1, r.prod_prologue ? 1 : 0, l);
        for (int i = 0; i < tt.n; i++) {
            tt.in_limb[i] = tt.out_limb[i] = tt.mod[i] = l[i].mod;
            tsv[i] = a.tin->ts[l[i].mod];
        }
        if (tt.n > 0)
            HIP_TRY(launch_tensor(be.qp, tt, tsv, a.tin->a0, a.tin->a1, a.tin->b0, a.tin->b1, View{nullptr, 0}, View{nullptr, 0}, cx, B, be.ctx->stream));
    }
    // base-2 gadget: bit windows of every Q-limb, NTT'd into every limb (evaluator_gadget_product.go:203-338)
    if (r.digits == KS_DIGITS_WINDOWS) return window_products_core(ev, levelQ, k, a, false);
    uint64_t *cxinv = be.ctx->arena_take(wq);
    uint64_t *dec = be.ctx->arena_take((size_t)B * bs);
    View inv{cxinv, (size_t)(levelQ + 1) * N};
    if (r.digits == KS_DIGITS_UNFUSED) {
        HIP_TRY(be_ntt(be, ident_tab(levelQ + 1), cx, inv, B, true, NTT_REDUCE_INPUT));
        TRY(decompose_ntt_into(ev, levelQ, levelP, levelP + 1, cx, inv, View{dec, bs}, ds, B));
        return ks_inner(ev, levelQ, levelP, View{dec, bs}, ds, k, a.c0Q, a.c0P, a.c1Q, a.c1P, B);
    }
    if (r.prod_prologue) {
        NttProdIn pin;
        pin.a = a.tin->a1; pin.b = a.tin->b1; pin.c = cx;
        for (int i = 0; i <= levelQ; i++) pin.ts[i] = a.tin->ts[i];
        HIP_TRY(launch_ntt_rows(be.qp, ident_tab(levelQ + 1), cx, inv, B, true, 0, be.ctx->stream, nullptr, &pin));
    } else {
        HIP_TRY(launch_ntt_rows(be.qp, ident_tab(levelQ + 1), cx, inv, B, true, a.cx_canonical ? 0 : NTT_REDUCE_INPUT, be.ctx->stream));
    }
    if (!r.mac_f64) {
        TRY(decompose_fused(ev, *c.dec, levelQ, levelP, levelP + 1, inv, View{dec, bs}, B));
        return ks_inner(ev, levelQ, levelP, View{dec, bs}, ds, k, a.c0Q, a.c0P, a.c1Q, a.c1P, B, &cx, levelP + 1, 0, 0, -1, a.giant);
    }
    // limbs below 2^47: NTT + MAC fused; the rest: row NTT then ks_inner.  The double-precision limbs of the decomposition are
    // read by ntt_mac_f64 only: they stay doubles in between
    int max_nsrc = 1;
    for (const FusedGroup &g : c.dec->groups) max_nsrc = std::max(max_nsrc, g.nsrc);
    const MacDigits digits{dec, bs, ds, f64_raw_ok(be, levelQ, levelP, max_nsrc), !a.cx_canonical};
    TRY(decompose_fused(ev, *c.dec, levelQ, levelP, levelP + 1, inv, View{dec, bs}, B, 1, digits.raw));
    TRY(ks_inner(ev, levelQ, levelP, View{dec, bs}, ds, k, a.c0Q, a.c0P, a.c1Q, a.c1P, B, &cx, levelP + 1, 1, 0, -1, a.giant));
    if (r.moddown == KS_MD_FUSED_MAC) {
        *a.pending = digits;
        return HE_OK;
    }
    return ks_mac_f64(ev, levelQ, k, r, a, digits, nullptr);
}
// The front of the fused ModDown for nb entries: INTT rows (P) -> [cols + ModUpPtoQ + cols] into sQ; the forward rows, with their
// epilogue, are the caller's (raw: they take NTT_INPUT_F64, the extension's doubles stay doubles).  canonical: accP is in [0, p)
int moddown_front_fused(Evaluator &ev, const FusedPlan &plan, int levelQ, int levelP, View accP, View sP, View sQ, int nb, bool canonical, bool *raw) {
    BasisExtender &be = *ev.be;
    hipStream_t st = be.ctx->stream;
    HIP_TRY(launch_ntt_rows(be.qp, ident_tab(levelP + 1, 0, 0, be.LQ), accP, sP, nb, true, canonical ? 0 : NTT_REDUCE_INPUT, st));
    const FusedGroup &g = plan.groups[0];
    *raw = f64_raw_ok(be, levelQ, -1, g.nsrc);
    HIP_TRY(launch_modup_fused(be.qp, g.dev, 1, g.nsrc, g.dst_classes, sP, sQ, sQ, nb, st, *raw, g.total_limbs));
    return HE_OK;
}
// the epilogue of those rows over the Q limbs of `tab`: out = (x - y) * P^-1 (addends, second component, tensor terms: the callers)
void moddown_epilogue(NttEpilogue &epi, const BasisExtender &be, int levelP, const LimbTab &tab, View y) {
    for (int i = 0; i < tab.n; i++) epi.s[i] = be.Q->moduli[tab.mod[i]] - be.md_ptoq[levelP][tab.mod[i]];
    epi.y = y; epi.has_w = false; epi.w = y;
}
// ModDownQPtoQNTT up to (not including) its last fused op: sQ = NTTLazy(ModUpPtoQ(INTTLazy(accP))) for nb entries.  No key here:
// fused exactly when the ModDown plan exists
int moddown_front(Evaluator &ev, int levelQ, int levelP, View accP, View sP, View sQ, int nb, bool canonical = false) {
    BasisExtender &be = *ev.be;
    const FusedPlan *plan = nullptr;
    TRY(get_md_plan(ev, levelQ, levelP, &plan));
    if (plan->ok) {
        bool raw = false;
        TRY(moddown_front_fused(ev, *plan, levelQ, levelP, accP, sP, sQ, nb, canonical, &raw));
        HIP_TRY(launch_ntt_rows(be.qp, ident_tab(levelQ + 1), sQ, sQ, nb, false, NTT_LAZY_OUT | (raw ? NTT_INPUT_F64 : 0), be.ctx->stream));
        return HE_OK;
    }
    HIP_TRY(be_ntt(be, ident_tab(levelP + 1, 0, 0, be.LQ), accP, sP, nb, true, NTT_REDUCE_INPUT));
    TRY(modup_between(be, false, levelP, levelQ, sP, sQ, 0, nb));
    const bool red = modup_out_needs_reduce(std::vector<uint64_t>(be.P->moduli.begin(), be.P->moduli.begin() + levelP + 1));
    HIP_TRY(be_ntt(be, ident_tab(levelQ + 1), sQ, sQ, nb, false, NTT_LAZY_OUT | (red ? NTT_REDUCE_INPUT : 0)));
    return HE_OK;
}
// last op of ModDown, optionally fused with the Ring.Add that every caller applies next:
// out = [add +] MRed(sQ + 2q - accQ, q - P^-1)
int moddown_back(Evaluator &ev, int levelQ, int levelP, View sQ, View accQ, View out, const View *add, int B) {
    BasisExtender &be = *ev.be;
    ScalarTab s{};
    for (int i = 0; i <= levelQ; i++) s.s[i] = be.Q->moduli[i] - be.md_ptoq[levelP][i];
    if (add) HIP_TRY(launch_ew_w(be.qp, ident_tab(levelQ + 1), EW_SUBMUL2Q_THEN_ADD, sQ, accQ, *add, out, B, &s, be.ctx->stream));
    else HIP_TRY(launch_ew(be.qp, ident_tab(levelQ + 1), EW_SUB_THEN_MUL_SCALAR_MONT_2Q, sQ, accQ, out, B, &s, nullptr, be.ctx->stream));
    return HE_OK;
}
// what a full gadget product runs on: out_k = [add_k +] GadgetProduct(cx)_k
struct GpArgs {
    const View *cx = nullptr, *hoisted = nullptr;  // the NTT-domain operand, or a hoisting buffer with its digits
    View out0, out1;
    int B = 0;
    const View *add0 = nullptr, *add1 = nullptr;
    bool cx_canonical = false;
    const TensorIn *tin = nullptr;  // with route.tensor_epilogue (no addends then)
    uint32_t scatter_ginv = 0;  // with KS_AUTO_EPILOGUE_SCATTER: g^-1 mod 2N, the epilogues store through it (NttEpilogue::scatter_ginv)
};
// full GadgetProduct.  Both components share every launch (accumulators are laid out [2][B] so ModDown runs once over 2B entries).
int gadget_product_core(Evaluator &ev, int levelQ, const Evk &k, const KsCall &c, const GpArgs &g) {
    BasisExtender &be = *ev.be;
    const KsRoute &r = c.route;
    const int levelP = k.nPk - 1, N = be.Q->N, B = g.B;
    const size_t sQw = (size_t)(levelQ + 1) * N, sPw = (size_t)(levelP + 1) * N;
    uint64_t *aQ = be.ctx->arena_take(2 * B * sQw), *aP = be.ctx->arena_take(2 * B * sPw);
    View a0Q{aQ, sQw}, a1Q{aQ + (size_t)B * sQw, sQw}, a0P{aP, sPw}, a1P{aP + (size_t)B * sPw, sPw};
    hipStream_t st = be.ctx->stream;
    if (r.moddown == KS_MD_NONE) {
        // no special primes: ModDown's levelP == -1 branch is a copy of the (canonical) Q accumulators (:76-81), followed by
        // the caller's Ring.Add where there is one
        TRY(gadget_product_lazy_core(ev, levelQ, k, c, LazyArgs{*g.cx, B, a0Q, View{nullptr, 0}, a1Q, View{nullptr, 0}, g.cx_canonical}));
        const LimbTab tq = ident_tab(levelQ + 1);
        HIP_TRY(launch_ew(be.qp, tq, g.add0 ? EW_ADD : EW_COPY, a0Q, g.add0 ? *g.add0 : a0Q, g.out0, B, nullptr, nullptr, st));
        HIP_TRY(launch_ew(be.qp, tq, g.add1 ? EW_ADD : EW_COPY, a1Q, g.add1 ? *g.add1 : a1Q, g.out1, B, nullptr, nullptr, st));
        return HE_OK;
    }
    const bool mac_epilogue = r.moddown == KS_MD_FUSED_MAC;
    MacDigits pending;
    const LazyArgs lazy{g.cx ? *g.cx : View{nullptr, 0}, B, a0Q, a0P, a1Q, a1P, g.cx_canonical, g.tin, nullptr, mac_epilogue ? &pending : nullptr};
    if (g.cx) TRY(gadget_product_lazy_core(ev, levelQ, k, c, lazy));
    else TRY(ks_inner(ev, levelQ, levelP, *g.hoisted, (size_t)(be.LQ + be.LP) * N, k, a0Q, a0P, a1Q, a1P, B));
    View sP{be.ctx->arena_take(2 * B * sPw), sPw}, sQ{be.ctx->arena_take(2 * B * sQw), sQw};
    if (r.moddown == KS_MD_UNFUSED) {
        TRY(moddown_front(ev, levelQ, levelP, View{aP, sPw}, sP, sQ, 2 * B, true));  // accumulators of ks_inner / ntt_mac: canonical
        TRY(moddown_back(ev, levelQ, levelP, sQ, a0Q, g.out0, g.add0, B));
        TRY(moddown_back(ev, levelQ, levelP, View{sQ.p + (size_t)B * sQw, sQw}, a1Q, g.out1, g.add1, B));
        return HE_OK;
    }
    // ModDown with every pass fused: INTT rows (P, both components) -> [cols + ModUpPtoQ + cols] -> NTT rows whose epilogue
    // applies (x - acc) * P^-1 and the caller's Add (or the tensor terms) and writes the final output.  With the MAC epilogue
    // those rows cover the Q limbs the integer kernels own; the NTT + MAC kernel does the same for the others.
    bool raw = false;
    TRY(moddown_front_fused(ev, *c.md, levelQ, levelP, View{aP, sPw}, sP, sQ, 2 * B, true, &raw));
    LimbTab ti;
    QPLimb l[kMaxLimbs];
    ti.n = qp_limbs(be, levelQ, -1, mac_epilogue ? 1 : 0, l);
    for (int i = 0; i < ti.n; i++) ti.in_limb[i] = ti.out_limb[i] = ti.mod[i] = l[i].mod;
    NttEpilogue epi;
    moddown_epilogue(epi, be, levelP, ti, a0Q);
    epi.scatter_ginv = g.scatter_ginv;
    epi.has_w = g.add0 != nullptr; epi.w = g.add0 ? *g.add0 : a0Q;
    epi.y_small_f64 = r.acc_q_f64;
    epi.zsplit = B; epi.out2 = g.out1; epi.y2 = a1Q; epi.has_w2 = g.add1 != nullptr; epi.w2 = g.add1 ? *g.add1 : a1Q;
    if (g.tin) {
        epi.tensor = true; epi.has_w = epi.has_w2 = false;
        epi.ta0 = g.tin->a0; epi.ta1 = g.tin->a1; epi.tb0 = g.tin->b0; epi.tb1 = g.tin->b1;
        for (int i = 0; i < ti.n; i++) epi.ts[i] = g.tin->ts[ti.mod[i]];
    }
    if (mac_epilogue) {
        NttMacEpilogue me;
        me.scatter_ginv = g.scatter_ginv;
        me.ext = sQ; me.ext_f64 = raw;
        me.out0 = g.out0; me.out1 = g.out1;
        me.has_w0 = g.add0 != nullptr && !g.tin; me.has_w1 = g.add1 != nullptr && !g.tin;
        me.w0 = g.add0 ? *g.add0 : g.out0; me.w1 = g.add1 ? *g.add1 : g.out1;
        me.tensor = g.tin != nullptr;
        if (g.tin) { me.ta0 = g.tin->a0; me.ta1 = g.tin->a1; me.tb0 = g.tin->b0; me.tb1 = g.tin->b1; }
        for (int i = 0; i <= levelQ; i++) {
            const ModConst &m = be.Q->sub[i].mc;
            me.sp[i] = (double)imform(be.Q->moduli[i] - be.md_ptoq[levelP][i], m.q, m.qinv);
            me.tsp[i] = g.tin ? (double)imform(imform(g.tin->ts[i], m.q, m.qinv), m.q, m.qinv) : 0.0;
        }
        TRY(ks_mac_f64(ev, levelQ, k, r, lazy, pending, &me));
    }
    if (ti.n > 0) HIP_TRY(launch_ntt_rows(be.qp, ti, sQ, g.out0, 2 * B, false, (raw && !mac_epilogue) ? NTT_INPUT_F64 : 0, st, &epi));
    return HE_OK;
}
// The route of one call of `form` with key k at levelQ: the facts are gathered here and nowhere else (each switch read once).
int ks_call(Evaluator &ev, KsForm form, int levelQ, const Evk &k, KsAlias alias, KsCall *out) {
    static const bool no_mac_epilogue = env_flag("HERING_NO_MAC_EPILOGUE");
    static const bool no_prod_prologue = env_flag("HERING_NO_PROD_PROLOGUE");
    static const bool no_tensor_epilogue = env_flag("HERING_NO_TENSOR_EPILOGUE");
    static const bool no_auto_scatter = env_flag("HERING_NO_AUTO_SCATTER");
    static const bool no_giant_fusion = env_flag("HERING_NO_GIANT_FUSION");
    const BasisExtender &be = *ev.be;
    const int logN = be.Q->logN;
    KsFacts f;
    f.form = form; f.ring_type = be.type; f.levelP = k.nPk - 1;
    f.pw2 = k.pw2 != 0; f.keyd = k.keyd != nullptr; f.f64_tables = be.d_twdi != nullptr;
    for (int j = 0; j < k.nPk; j++) f.p_class2 = f.p_class2 || be.small[be.LQ + j] == 2;
    // (only the plans the form's launches and tables_ok ask about)
    const bool lazy = form == KS_LAZY || form == KS_GIANT_STEP || form == KS_AUTOMORPHISM_HOISTED_LAZY;
    if (k.nPk > 0 && !k.pw2 && form != KS_HOISTED && form != KS_AUTOMORPHISM_HOISTED_LAZY) TRY(get_dec_plan(ev, levelQ, k.nPk - 1, k.nPk, &out->dec));
    if (k.nPk > 0 && !lazy) TRY(get_md_plan(ev, levelQ, k.nPk - 1, &out->md));
    f.dec_ok = out->dec && out->dec->ok; f.md_ok = out->md && out->md->ok;
    f.prod_in_supported = ntt_prod_in_supported(logN); f.scatter_supported = epilogue_scatter_supported(logN);
    f.mac_epilogue_supported = ntt_mac_epilogue_supported(logN); f.mac_giant_supported = ntt_mac_giant_supported(logN);
    f.alias = alias;
    f.no_mac_epilogue = no_mac_epilogue; f.no_prod_prologue = no_prod_prologue; f.no_tensor_epilogue = no_tensor_epilogue;
    f.no_auto_scatter = no_auto_scatter; f.no_giant_fusion = no_giant_fusion;
    out->route = ks_route(f);
    return HE_OK;
}
// a full key switch of `form`: its route, then its launches
int key_switch(Evaluator &ev, KsForm form, int levelQ, const Evk &k, KsAlias alias, const GpArgs &g) {
    KsCall c;
    TRY(ks_call(ev, form, levelQ, k, alias, &c));
    return gadget_product_core(ev, levelQ, k, c, g);
}
// What every key-switch request starts with, and its tables_ok from the route of `form` (KS_FORM_COUNT: the entry sets its own)
void ks_request(CoReq &q, int op, std::shared_ptr<Evaluator> ev, std::shared_ptr<Evk> k, int level, KsForm form, KsAlias alias) {
    q.op = op; q.obj = ev.get(); q.key = k.get(); q.par[0] = level;
    q.keep.push_back(ev); q.keep.push_back(k);
    if (!k || form == KS_FORM_COUNT) return;
    q.tables_ok = [ev, k, form, level, alias](bool *ok) -> int {
        KsCall c;
        TRY(ks_call(*ev, form, level, *k, alias, &c));
        *ok = c.route.tables_ok;
        return HE_OK;
    };
}
int check_key(const Evaluator &ev, const Evk &k, int &levelQ, const char *who) {
    if (k.ev.get() != &ev) return fail(HE_EINVAL, "%s: key belongs to another evaluator", who);
    if (levelQ < 0) return fail(HE_EINVAL, "%s: negative level", who);
    levelQ = std::min(levelQ, k.nQk - 1);  // utils.Min(levelQ, gadgetCt.LevelQ())
    return HE_OK;
}
// a hoisting buffer is only meaningful for the evaluator and the (levelQ, levelP) digits it was filled at
int check_decomp(const Evaluator &ev, const Decomp &dec, int levelQ, int levelP, const char *who) {
    if (dec.ev.get() != &ev) return fail(HE_EINVAL, "%s: decomposition buffer belongs to another evaluator", who);
    if (dec.fillQ < 0) return fail(HE_EINVAL, "%s: decomposition buffer was never filled", who);
    if (levelP != dec.fillP || levelQ > dec.fillQ || base_rns_size(levelQ, levelP) > dec.fill_beta)
        return fail(HE_EINVAL, "%s: decomposition buffer holds %d digits of level (%d,%d), (%d,%d) requested", who, dec.fill_beta,
                    dec.fillQ, dec.fillP, levelQ, levelP);
    return HE_OK;
}
}  // namespace

// limbs of an evaluation key's 2 beta rows at (levelQ, levelP): read once per call, shared by the batch
static double key_limbs(const Evk &k, int levelQ) { return 2.0 * key_beta(k, levelQ) * (levelQ + k.nPk + 1); }
// What every full key switch (gadget_product_core) starts with: the bytes it moves (`limbs` polynomial limbs per entry and the
// key), its arithmetic, and its scratch plus `extra` words of the caller's.  decompose: the operand is decomposed here (false:
// a hoisting buffer holds its digits).
static int keyswitch_begin(Evaluator &ev, const Evk &k, int level, double limbs, bool decompose, int B, size_t extra = 0) {
    BasisExtender &be = *ev.be;
    be.ctx->acct(limbs, key_limbs(k, level), B, be.Q->N);
    { Valu V(be.Q->logN); valu_gadget_product(V, be, level, k.nPk - 1, key_beta(k, level), decompose); V.into(*be.ctx, B); }
    return be.ctx->arena_reserve(ks_scratch_words(be, level, k.nPk - 1, B, decompose, &k) + extra);
}
int he_gadget_product_lazy(he_handle hev, int levelQ, he_handle hcx, he_handle hk, he_handle c0Q, he_handle c0P, he_handle c1Q, he_handle c1P) {
    GET(ev, Evaluator, hev, T_EVAL);
    GET(k, Evk, hk, T_EVK);
    BasisExtender &be = *ev->be;
    TRY(check_key(*ev, *k, levelQ, "he_gadget_product_lazy"));
    CoReq q;
    Operands o(q, "he_gadget_product_lazy", be);
    o.in(hcx, levelQ + 1, "cx");
    o.qp(true, c0Q, c0P, c1Q, c1P, levelQ, k->nPk - 1);
    TRY(o.check());
    ks_request(q, CO_GP_LAZY, ev, k, levelQ, KS_LAZY, KsAlias{});
    q.run = [ev, k, levelQ](const View *v, int B) -> int {
        BasisExtender &be = *ev->be;
        be.ctx->acct(levelQ + 1 + 2.0 * (levelQ + k->nPk + 1), key_limbs(*k, levelQ), B, be.Q->N);  // cx in, two QP accumulators out, key
        { Valu V(be.Q->logN); valu_keyswitch(V, be, levelQ, k->nPk - 1, key_beta(*k, levelQ), true, true); V.into(*be.ctx, B); }
        TRY(be.ctx->arena_reserve(ks_scratch_words(be, levelQ, k->nPk - 1, B, true, k.get())));
        KsCall c;
        TRY(ks_call(*ev, KS_LAZY, levelQ, *k, KsAlias{}, &c));
        return gadget_product_lazy_core(*ev, levelQ, *k, c, LazyArgs{v[0], B, v[1], v[2], v[3], v[4]});
    };
    return co_dispatch(*be.ctx, o.B, q);
}
int he_gadget_product_hoisted_lazy(he_handle hev, int levelQ, he_handle hdec, he_handle hk, he_handle c0Q, he_handle c0P, he_handle c1Q, he_handle c1P) {
    GET(ev, Evaluator, hev, T_EVAL);
    GET(dec, Decomp, hdec, T_DECOMP);
    GET(k, Evk, hk, T_EVK);
    BasisExtender &be = *ev->be;
    TRY(check_key(*ev, *k, levelQ, "he_gadget_product_hoisted_lazy"));
    if (k->pw2) return fail(HE_EINVAL, "he_gadget_product_hoisted_lazy: method is unsupported for BaseTwoDecomposition != 0");
    TRY(check_decomp(*ev, *dec, levelQ, k->nPk - 1, "he_gadget_product_hoisted_lazy"));
    CoReq q;
    Operands o(q, "he_gadget_product_hoisted_lazy", be, dec->batch);
    o.raw(dec->view(), dec);
    o.qp(true, c0Q, c0P, c1Q, c1P, levelQ, k->nPk - 1);
    TRY(o.check());
    const size_t dec_ds = dec->dstride();
    ks_request(q, CO_GP_HOISTED_LAZY, ev, k, levelQ, KS_FORM_COUNT, KsAlias{});
    q.run = [ev, k, levelQ, dec_ds](const View *v, int B) -> int {
        BasisExtender &be = *ev->be;
        be.ctx->acct(key_limbs(*k, levelQ) / 2 + 2.0 * (levelQ + k->nPk + 1), key_limbs(*k, levelQ), B, be.Q->N);  // decomposition in, accumulators out, key
        { Valu V(be.Q->logN); valu_keyswitch(V, be, levelQ, k->nPk - 1, base_rns_size(levelQ, k->nPk - 1), false, true); V.into(*be.ctx, B); }
        return ks_inner(*ev, levelQ, k->nPk - 1, v[0], dec_ds, *k, v[1], v[2], v[3], v[4], B);
    };
    return co_dispatch(*be.ctx, dec->batch, q);
}
int he_gadget_product_hoisted_lazy_digits(he_handle hev, int levelQ, he_handle hdec, he_handle hk, int digit_begin, int digit_end,
                                          he_handle c0Q, he_handle c0P, he_handle c1Q, he_handle c1P) {
    const char *who = "he_gadget_product_hoisted_lazy_digits";
    GET(ev, Evaluator, hev, T_EVAL);
    GET(dec, Decomp, hdec, T_DECOMP);
    GET(k, Evk, hk, T_EVK);
    BasisExtender &be = *ev->be;
    TRY(check_key(*ev, *k, levelQ, who));
    if (k->pw2) return fail(HE_EINVAL, "%s: method is unsupported for BaseTwoDecomposition != 0", who);
    TRY(check_decomp(*ev, *dec, levelQ, k->nPk - 1, who));
    const int beta = base_rns_size(levelQ, k->nPk - 1);
    if (digit_begin < 0 || digit_end > beta || digit_begin > digit_end) return fail(HE_EINVAL, "%s: digits [%d,%d) outside [0,%d)", who, digit_begin, digit_end, beta);
    CoReq q;  // (not filed: the launches below are made at once; the request only carries the operands' views)
    Operands o(q, who, be, dec->batch);
    o.qp(true, c0Q, c0P, c1Q, c1P, levelQ, k->nPk - 1);
    TRY(o.check());
    Scope sc(be.ctx.get());
    be.ctx->acct((double)(digit_end - digit_begin) * (levelQ + k->nPk + 1) + 2.0 * (levelQ + k->nPk + 1),
                 2.0 * (digit_end - digit_begin) * (levelQ + k->nPk + 1), dec->batch, be.Q->N);
    if (digit_begin == digit_end) {  // an empty share contributes zero -- to the limbs a non-empty share writes (levels + 1), not above
        const int lv[4] = {levelQ + 1, k->nPk, levelQ + 1, k->nPk};
        for (int i = 0; i < 4; i++) {
            const Poly *pp = o.ops[i].p;
            HIP_TRY(hipMemset2DAsync(pp->d, (size_t)pp->nlimbs * pp->N * 8, 0, (size_t)lv[i] * pp->N * 8, pp->batch, be.ctx->stream));
        }
        return HE_OK;
    }
    return ks_inner(*ev, levelQ, k->nPk - 1, dec->view(), dec->dstride(), *k, q.ops[0], q.ops[1], q.ops[2], q.ops[3], dec->batch, nullptr, 0, 0,
                    digit_begin, digit_end);
}
int he_moddown(he_handle hev, int levelQ, int levelP, he_handle c0Q, he_handle c0P, he_handle c1Q, he_handle c1P, he_handle hout0, he_handle hout1) {
    GET(ev, Evaluator, hev, T_EVAL);
    GET(out0, Poly, hout0, T_POLY);
    GET(out1, Poly, hout1, T_POLY);
    BasisExtender &be = *ev->be;
    if (levelQ < 0 || levelQ >= be.LQ || levelP < -1 || levelP >= be.LP) return fail(HE_EINVAL, "he_moddown: level out of range");
    if (levelP == -1) {  // ModDown without special primes, NTT -> NTT: ctQP.Value[k].Q.CopyLvl(levelQ, ct.Value[k]) (:76-81)
        CoReq q;
        Operands o(q, "he_moddown", be, out0->batch);
        const int i0 = o.in(c0Q, levelQ + 1, "c0Q"), i1 = o.in(c1Q, levelQ + 1, "c1Q");
        // out_k may be c_kQ (the reference's ModDown runs component by component); out_k == c_{1-k}Q is not in place
        o.inplace(o.out(out0, levelQ + 1, "out0"), i0);
        o.inplace(o.out(out1, levelQ + 1, "out1"), i1);
        TRY(o.check());
        q.op = CO_MODDOWN; q.obj = ev.get(); q.par[0] = levelQ; q.par[1] = -1;
        q.keep.push_back(ev);
        q.run = [ev, levelQ](const View *v, int B) -> int {
            BasisExtender &be = *ev->be;
            be.ctx->acct(4.0 * (levelQ + 1), 0, B, be.Q->N);
            const LimbTab tq = ident_tab(levelQ + 1);
            HIP_TRY(launch_ew(be.qp, tq, EW_COPY, v[0], v[0], v[2], B, nullptr, nullptr, be.ctx->stream));
            HIP_TRY(launch_ew(be.qp, tq, EW_COPY, v[1], v[1], v[3], B, nullptr, nullptr, be.ctx->stream));
            return HE_OK;
        };
        return co_dispatch(*be.ctx, out0->batch, q);
    }
    CoReq q;
    Operands o(q, "he_moddown", be, out0->batch);
    const int ic = o.qp(false, c0Q, c0P, c1Q, c1P, levelQ, levelP);
    o.inplace(o.out(out0, levelQ + 1, "out0"), ic);
    o.inplace(o.out(out1, levelQ + 1, "out1"), ic + 2);
    TRY(o.check());
    q.op = CO_MODDOWN; q.obj = ev.get(); q.par[0] = levelQ; q.par[1] = levelP;
    q.keep.push_back(ev);
    q.run = [ev, levelQ, levelP](const View *v, int B) -> int {
        BasisExtender &be = *ev->be;
        be.ctx->acct(2.0 * (2.0 * (levelQ + 1) + levelP + 1), 0, B, be.Q->N);  // ModDown of both components: 2 (2 L + alpha)
        { Valu V(be.Q->logN); valu_moddown(V, be, levelQ, levelP); valu_moddown(V, be, levelQ, levelP); V.into(*be.ctx, B); }
        TRY(be.ctx->arena_reserve(ks_scratch_words(be, levelQ, levelP, B, false)));
        const size_t sPw = (size_t)(levelP + 1) * be.Q->N, sQw = (size_t)(levelQ + 1) * be.Q->N;
        View sP{be.ctx->arena_take(B * sPw), sPw}, sQ{be.ctx->arena_take(B * sQw), sQw};
        for (int c = 0; c < 2; c++) {  // component by component, as the reference
            TRY(moddown_front(*ev, levelQ, levelP, v[2 * c + 1], sP, sQ, B));
            TRY(moddown_back(*ev, levelQ, levelP, sQ, v[2 * c], v[4 + c], nullptr, B));
        }
        return HE_OK;
    };
    q.tables_ok = [ev](bool *ok) -> int { *ok = ev->be->type == 0; return HE_OK; };
    return co_dispatch(*be.ctx, out0->batch, q);
}
// the launches of ModDownQPtoQNTT over B entries: v = (p1Q, p1P, p2Q); p2Q may be p1Q.  The caller holds the context (Scope).
static int eval_moddown_run(const std::shared_ptr<Evaluator> &ev, int levelQ, int levelP, const View *v, int B) {
    BasisExtender &be = *ev->be;
    const int N = be.Q->N;
    be.ctx->acct(2.0 * (levelQ + 1) + levelP + 1, 0, B, N);  // ModDownQPtoQNTT: 2 L + alpha
    { Valu V(be.Q->logN); valu_moddown(V, be, levelQ, levelP); V.into(*be.ctx, B); }
    const size_t wP = (size_t)B * (levelP + 1) * N, wQ = (size_t)B * (levelQ + 1) * N;
    TRY(be.ctx->arena_reserve(eval_moddown_words(be, levelQ, levelP, B)));
    View sP{be.ctx->arena_take(wP), (size_t)(levelP + 1) * N};
    View sQ{be.ctx->arena_take(wQ), (size_t)(levelQ + 1) * N};
    const FusedPlan *plan = nullptr;
    TRY(get_md_plan(*ev, levelQ, levelP, &plan));
    // the fused basis extension runs one 128-thread workgroup per 1024 coefficients and batch entry over ALL destination
    // limbs: below one workgroup per CU the six-launch path, which also spreads the limbs over the grid, has the lower latency
    const int rowbits = ntt_row_bits(be.Q->logN);
    const bool wide = (size_t)B * ((size_t)1 << rowbits) / 128 >= 256;
    if (!plan->ok || !wide) return moddown_q_ntt(be, levelQ, levelP, v[0], v[1], v[2], B, sP, sQ);
    // three launches: INTT rows (P) -> [cols + ModUpPtoQ + cols] -> NTT rows whose epilogue is the last op of the ModDown
    bool raw = false;
    TRY(moddown_front_fused(*ev, *plan, levelQ, levelP, v[1], sP, sQ, B, false, &raw));
    const LimbTab tq = ident_tab(levelQ + 1);
    NttEpilogue epi;
    moddown_epilogue(epi, be, levelP, tq, v[0]);
    epi.y_reduce = true;  // p1Q is the caller's: any 64-bit word
    HIP_TRY(launch_ntt_rows(be.qp, tq, sQ, v[2], B, false, raw ? NTT_INPUT_F64 : 0, be.ctx->stream, &epi));
    return HE_OK;
}
int he_eval_moddown_qp_to_q_ntt(he_handle hev, int levelQ, int levelP, he_handle h1q, he_handle h1p, he_handle h2) {
    GET(ev, Evaluator, hev, T_EVAL);
    BasisExtender &be = *ev->be;
    const char *who = "he_eval_moddown_qp_to_q_ntt";
    if (levelQ < 0 || levelQ >= be.LQ || levelP < 0 || levelP >= be.LP) return fail(HE_EINVAL, "%s: level out of range", who);
    CoReq q;
    Operands o(q, who, be);
    const int iq = o.in(h1q, levelQ + 1);
    o.inP(h1p, levelP + 1);
    o.inplace(o.out(h2, levelQ + 1), iq);
    TRY(o.check());
    q.op = CO_EVAL_MODDOWN; q.obj = ev.get(); q.par[0] = levelQ; q.par[1] = levelP;
    q.keep.push_back(ev);
    q.run = [ev, levelQ, levelP](const View *v, int B) -> int { return eval_moddown_run(ev, levelQ, levelP, v, B); };
    q.tables_ok = [ev](bool *ok) -> int { *ok = ev->be->type == 0; return HE_OK; };
    return co_dispatch(*be.ctx, o.B, q);
}
int he_gadget_product(he_handle hev, int levelQ, he_handle hcx, he_handle hk, he_handle hout0, he_handle hout1) {
    GET(ev, Evaluator, hev, T_EVAL);
    GET(k, Evk, hk, T_EVK);
    BasisExtender &be = *ev->be;
    TRY(check_key(*ev, *k, levelQ, "he_gadget_product"));
    CoReq q;
    Operands o(q, "he_gadget_product", be);
    const int ix = o.in(hcx, levelQ + 1, "cx"), i0 = o.out(hout0, levelQ + 1, "out0"), i1 = o.out(hout1, levelQ + 1, "out1");
    o.all_inplace = true;
    TRY(o.check());
    // an output that is the key switch's NTT-domain operand: its own-digit limbs are still being read while the fused epilogue
    // writes the outputs of OTHER entries' workgroups -- such requests (their own key: the aliasing pattern) are served one by one
    const KsAlias alias{o.same(ix, i0) || o.same(ix, i1)};
    ks_request(q, CO_GADGET_PRODUCT, ev, k, levelQ, KS_GADGET_PRODUCT, alias);
    q.run = [ev, k, levelQ, alias](const View *v, int B) -> int {
        TRY(keyswitch_begin(*ev, *k, levelQ, 3.0 * (levelQ + 1), true, B));  // GadgetProduct: 3 L + 2 beta (L + alpha)
        return key_switch(*ev, KS_GADGET_PRODUCT, levelQ, *k, alias, GpArgs{&v[0], nullptr, v[1], v[2], B});
    };
    return co_dispatch(*be.ctx, o.B, q);
}
int he_gadget_product_hoisted(he_handle hev, int levelQ, he_handle hdec, he_handle hk, he_handle hout0, he_handle hout1) {
    GET(ev, Evaluator, hev, T_EVAL);
    GET(dec, Decomp, hdec, T_DECOMP);
    GET(k, Evk, hk, T_EVK);
    BasisExtender &be = *ev->be;
    TRY(check_key(*ev, *k, levelQ, "he_gadget_product_hoisted"));
    if (k->pw2) return fail(HE_EINVAL, "he_gadget_product_hoisted: method is unsupported for BaseTwoDecomposition != 0");
    TRY(check_decomp(*ev, *dec, levelQ, k->nPk - 1, "he_gadget_product_hoisted"));
    CoReq q;
    Operands o(q, "he_gadget_product_hoisted", be, dec->batch);
    o.raw(dec->view(), dec);
    o.out(hout0, levelQ + 1, "out0");
    o.out(hout1, levelQ + 1, "out1");
    TRY(o.check());
    ks_request(q, CO_GP_HOISTED, ev, k, levelQ, KS_HOISTED, KsAlias{});
    q.run = [ev, k, levelQ](const View *v, int B) -> int {
        TRY(keyswitch_begin(*ev, *k, levelQ, key_limbs(*k, levelQ) / 2 + 2.0 * (levelQ + 1), false, B));  // hoisted: decomposition in, 2 L out, key
        return key_switch(*ev, KS_HOISTED, levelQ, *k, KsAlias{}, GpArgs{nullptr, &v[0], v[1], v[2], B});
    };
    return co_dispatch(*be.ctx, dec->batch, q);
}

// Relinearize (core/rlwe/evaluator_evaluationkey.go:117-148)
int he_relinearize(he_handle hev, int level, he_handle hin0, he_handle hin1, he_handle hin2, he_handle hk, he_handle hout0, he_handle hout1) {
    GET(ev, Evaluator, hev, T_EVAL);
    GET(k, Evk, hk, T_EVK);
    BasisExtender &be = *ev->be;
    TRY(check_key(*ev, *k, level, "he_relinearize"));
    CoReq q;
    Operands o(q, "he_relinearize", be);
    const int i0 = o.in(hin0, level + 1, "in0"), i1 = o.in(hin1, level + 1, "in1"), i2 = o.in(hin2, level + 1, "in2");
    const int o0 = o.out(hout0, level + 1, "out0"), o1 = o.out(hout1, level + 1, "out1");
    o.all_inplace = true;
    TRY(o.check());
    // crossed: an output is the OTHER component's addend -- the separate launches would write it before that component reads it,
    // so the addends are staged first
    const bool cross = o.same(i0, o1) || o.same(i1, o0);
    // Aliasing that the batched pipeline cannot take for a whole batch: an output that is the key switch's NTT-domain operand
    // (in2) or the OTHER component's addend.  An output equal to its own component's addend -- Relinearize in place -- is read and
    // written by the same thread and batches normally.
    const KsAlias alias{o.same(i2, o0) || o.same(i2, o1), false, cross};
    ks_request(q, CO_RELINEARIZE, ev, k, level, KS_GADGET_PRODUCT, alias);
    q.run = [ev, k, level, cross, alias](const View *v, int B) -> int {
        BasisExtender &be = *ev->be;
        const size_t wQ = (size_t)B * (level + 1) * be.Q->N;
        TRY(keyswitch_begin(*ev, *k, level, 5.0 * (level + 1), true, B, cross ? 2 * wQ + 4 : 0));  // Relinearize: 3 L in, 2 L out, key
        View a0 = v[0], a1 = v[1];
        if (cross) {  // (served one by one: plain views)
            a0 = View{be.ctx->arena_take(wQ), (size_t)(level + 1) * be.Q->N}; a1 = View{be.ctx->arena_take(wQ), a0.bstride};
            HIP_TRY(launch_ew(be.qp, ident_tab(level + 1), EW_COPY, v[0], v[0], a0, B, nullptr, nullptr, be.ctx->stream));
            HIP_TRY(launch_ew(be.qp, ident_tab(level + 1), EW_COPY, v[1], v[1], a1, B, nullptr, nullptr, be.ctx->stream));
        }
        return key_switch(*ev, KS_GADGET_PRODUCT, level, *k, alias, GpArgs{&v[2], nullptr, v[3], v[4], B, &a0, &a1});
    };
    return co_dispatch(*be.ctx, o.B, q);
}

// Automorphism / AutomorphismHoisted (core/rlwe/evaluator_automorphism.go:13-100), NTT domain
// the evaluator's cached index table of a Galois element (built once, on the context's stream: later launches are ordered after it)
static int cached_auto_index(Evaluator &ev, uint64_t gal, const uint32_t **out) {
    auto it = ev.auto_index.find(gal);
    if (it != ev.auto_index.end()) { *out = it->second; return HE_OK; }
    BasisExtender &be = *ev.be;
    // a bound on the memory a long-running caller can pin -- but never while a hipGraph of this context is alive or being
    // recorded: captured Automorphism launches have these device pointers baked into their kernel nodes (and a stream
    // synchronisation would invalidate a capture in progress); the cache then grows past the bound until the graphs are gone
    if (ev.auto_index.size() >= Evaluator::kAutoIndexCap && be.ctx->live_graphs == 0 && !be.ctx->capturing) {
        HIP_TRY(hipStreamSynchronize(be.ctx->stream));
        for (auto &kv : ev.auto_index) (void)hipFree(kv.second);
        ev.auto_index.clear();
    }
    uint32_t *d = nullptr;
    HIP_TRY(hipMalloc((void **)&d, (size_t)be.Q->N * sizeof(uint32_t)));
    hipError_t e = launch_build_automorphism_index(be.Q->logN, be.Q->logN + be.type, gal, d, be.ctx->stream);
    if (e != hipSuccess) { (void)hipFree(d); return fail(HE_EDEVICE, "automorphism index: %s", hipGetErrorString(e)); }
    ev.auto_index.emplace(gal, d);
    *out = d;
    return HE_OK;
}
// the launches of Automorphism / AutomorphismHoisted over B entries; the caller holds the context (Scope).  in1: the NTT-domain
// second component (null when `dec` holds its decomposition).  in0 / in1 / out0 / out1 may carry entry tables (a coalesced batch)
// when the route said so.
static int automorphism_core(Evaluator &ev, int level, View in0, const View *in1, const View *dec, uint64_t gal, const Evk &k, View out0,
                             View out1, int B, KsAlias alias) {
    BasisExtender &be = *ev.be;
    const int N = be.Q->N;
    const size_t wQ = (size_t)B * (level + 1) * N;
    // Rotate: (4 L + 2 beta (L + alpha)); hoisted: the decomposition replaces the second input
    TRY(keyswitch_begin(ev, k, level, dec ? 3.0 * (level + 1) + key_limbs(k, level) / 2 : 4.0 * (level + 1), !dec, B, 2 * wQ + (size_t)N));
    KsCall c;
    TRY(ks_call(ev, dec ? KS_AUTOMORPHISM_HOISTED : KS_AUTOMORPHISM, level, k, alias, &c));
    GpArgs g{in1, dec, out0, out1, B, &in0};
    // the automorphism is applied where the key switch writes its result ...
    if (c.route.automorphism == KS_AUTO_EPILOGUE_SCATTER) {
        g.scatter_ginv = galois_inverse(gal, be.Q->logN);
        return gadget_product_core(ev, level, k, c, g);
    }
    // ... or by two gather passes over the intermediate ciphertext
    View t0{be.ctx->arena_take(wQ), (size_t)(level + 1) * N}, t1{be.ctx->arena_take(wQ), (size_t)(level + 1) * N};
    const uint32_t *index = nullptr;
    TRY(cached_auto_index(ev, gal, &index));
    g.out0 = t0; g.out1 = t1;
    TRY(gadget_product_core(ev, level, k, c, g));
    HIP_TRY(launch_gather(be.qp, ident_tab(level + 1), t0, index, out0, B, false, be.ctx->stream));
    HIP_TRY(launch_gather(be.qp, ident_tab(level + 1), t1, index, out1, B, false, be.ctx->stream));
    return HE_OK;
}
static int automorphism_common(he_handle hev, int level, he_handle hin0, he_handle hin1, he_handle hdec, uint64_t gal, he_handle hk,
                               he_handle hout0, he_handle hout1, const char *who) {
    GET(ev, Evaluator, hev, T_EVAL);
    GET(k, Evk, hk, T_EVK);
    std::shared_ptr<Decomp> dec;
    if (hdec) { dec = get<Decomp>(hdec, T_DECOMP); if (!dec) return fail(HE_EHANDLE, "%s: bad decomposition handle", who); }
    BasisExtender &be = *ev->be;
    TRY(check_key(*ev, *k, level, who));
    const bool hoisted = dec != nullptr;
    CoReq q;
    Operands o(q, who, be, hoisted ? dec->batch : Operands::kCall);
    const int i0 = o.in(hin0, level + 1, "in0"), i1 = hoisted ? o.raw(dec->view(), dec) : o.in(hin1, level + 1, "in1");
    const int o0 = o.out(hout0, level + 1, "out0"), o1 = o.out(hout1, level + 1, "out1");
    o.all_inplace = true;
    TRY(o.check());
    if (!(gal & 1)) return fail(HE_EINVAL, "%s: Galois element must be odd", who);
    if (dec && k->pw2) return fail(HE_EINVAL, "%s: method is unsupported for BaseTwoDecomposition != 0", who);
    if (dec) TRY(check_decomp(*ev, *dec, level, k->nPk - 1, who));
    gal = reduce_gal(gal, be.Q->logN, be.type);
    // (an automorphism that writes onto its own inputs takes the gather form, which reads them all first: no entry tables then)
    const KsAlias alias{o.same(i1, o0) || o.same(i1, o1), o.same(i0, o0), o.same(i0, o1)};
    ks_request(q, hoisted ? CO_AUTO_HOISTED : CO_AUTOMORPHISM, ev, k, level, hoisted ? KS_AUTOMORPHISM_HOISTED : KS_AUTOMORPHISM, alias); q.par[1] = (int64_t)gal;
    q.run = [ev, k, level, gal, hoisted, alias](const View *v, int B) -> int {
        return automorphism_core(*ev, level, v[0], hoisted ? nullptr : &v[1], hoisted ? &v[1] : nullptr, gal, *k, v[2], v[3], B, alias);
    };
    return co_dispatch(*be.ctx, o.B, q);
}
int he_automorphism_ct(he_handle ev, int level, he_handle in0, he_handle in1, uint64_t gal, he_handle gk, he_handle out0, he_handle out1) {
    return automorphism_common(ev, level, in0, in1, 0, gal, gk, out0, out1, "he_automorphism_ct");
}
int he_automorphism_hoisted(he_handle ev, int level, he_handle in0, he_handle dec, uint64_t gal, he_handle gk, he_handle out0, he_handle out1) {
    if (!dec) return fail(HE_EHANDLE, "he_automorphism_hoisted: null decomposition handle");
    return automorphism_common(ev, level, in0, 0, dec, gal, gk, out0, out1, "he_automorphism_hoisted");
}

// AutomorphismHoistedLazy (core/rlwe/evaluator_automorphism.go:104-165), NTT domain
static int auto_hoisted_lazy_run(const std::shared_ptr<Evaluator> &ev, const std::shared_ptr<Evk> &k, int levelQ, int levelP, uint64_t gal,
                                 KsAlias alias, size_t dec_ds, const View *v, int B);
int he_automorphism_hoisted_lazy(he_handle hev, int levelQ, he_handle hin0, he_handle hdec, uint64_t gal, he_handle hk, he_handle c0Q,
                                 he_handle c0P, he_handle c1Q, he_handle c1P) {
    GET(ev, Evaluator, hev, T_EVAL);
    GET(dec, Decomp, hdec, T_DECOMP);
    GET(k, Evk, hk, T_EVK);
    BasisExtender &be = *ev->be;
    if (levelQ < 0 || levelQ > k->nQk - 1) return fail(HE_EINVAL, "he_automorphism_hoisted_lazy: levelQ out of range");
    const int levelP = k->nPk - 1, B = dec->batch;
    if (k->ev.get() != ev.get()) return fail(HE_EINVAL, "he_automorphism_hoisted_lazy: key belongs to another evaluator");
    if (k->pw2) return fail(HE_EINVAL, "he_automorphism_hoisted_lazy: method is unsupported for BaseTwoDecomposition != 0");
    if (!(gal & 1)) return fail(HE_EINVAL, "he_automorphism_hoisted_lazy: Galois element must be odd");
    TRY(check_decomp(*ev, *dec, levelQ, levelP, "he_automorphism_hoisted_lazy"));
    CoReq q;
    Operands o(q, "he_automorphism_hoisted_lazy", be, B);
    const int ii = o.in(hin0, levelQ + 1, "in0");
    o.raw(dec->view(), dec);
    const int ic = o.qp(true, c0Q, c0P, c1Q, c1P, levelQ, levelP);
    // a Q output may be in0 (read before it is written: the gather form below)
    o.inplace(ic, ii);
    o.inplace(ic + 2, ii);
    TRY(o.check());
    gal = reduce_gal(gal, be.Q->logN, be.type);
    const KsAlias alias{false, o.same(ic, ii), o.same(ic + 2, ii)};
    const size_t dec_ds = dec->dstride();
    ks_request(q, CO_AUTO_HOISTED_LAZY, ev, k, levelQ, KS_FORM_COUNT, KsAlias{}); q.par[1] = (int64_t)gal;
    q.run = [ev, k, levelQ, levelP, gal, alias, dec_ds](const View *v, int B) -> int {
        return auto_hoisted_lazy_run(ev, k, levelQ, levelP, gal, alias, dec_ds, v, B);
    };
    return co_dispatch(*be.ctx, B, q);
}
// the launches of AutomorphismHoistedLazy over B entries: v = (in0, the hoisting buffer, c0Q, c0P, c1Q, c1P).  The caller holds
// the context (Scope).
static int auto_hoisted_lazy_run(const std::shared_ptr<Evaluator> &ev, const std::shared_ptr<Evk> &k, int levelQ, int levelP, uint64_t gal,
                                 KsAlias alias, size_t dec_ds, const View *v, int B) {
    BasisExtender &be = *ev->be;
    const int N = be.Q->N;
    be.ctx->acct(levelQ + 1 + key_limbs(*k, levelQ) / 2 + 2.0 * (levelQ + levelP + 2), key_limbs(*k, levelQ), B, N);
    { Valu V(be.Q->logN); valu_keyswitch(V, be, levelQ, levelP, base_rns_size(levelQ, levelP), false, true); for (int i = 0; i <= levelQ; i++) V.mul(cls_f64(be.small, i), 1.0); V.into(*be.ctx, B); }
    ScalarTab s{};  // ctTmp[1].Q = ctIn[0] * P   (MulScalarBigint with P = prod p_j at levelP)
    for (int i = 0; i <= levelQ; i++) {
        const ModConst &m = be.Q->sub[i].mc;
        uint64_t pm = 1;
        for (int j = 0; j <= levelP; j++) pm = mulmod(pm, be.P->moduli[j] % m.q, m.q);
        s.s[i] = mform(pm, m.q, m.brc0, m.brc1);
    }
    // ONE launch: the key inner product adds ctIn[0] * P to component 0 at the source position and stores all four accumulators
    // through the automorphism (KsScatter) -- instead of inner product, two element-wise passes and four gathers.  Standard
    // ring, and the outputs must not be the addend (other threads still read it).
    KsCall c;
    TRY(ks_call(*ev, KS_AUTOMORPHISM_HOISTED_LAZY, levelQ, *k, alias, &c));
    if (c.route.automorphism == KS_AUTO_KS_SCATTER) {
        KsScatter ks;
        ks.ginv = galois_inverse(gal, be.Q->logN);
        ks.add0 = v[0];
        for (int i = 0; i <= levelQ; i++) ks.add_s[i] = s.s[i];
        return ks_inner(*ev, levelQ, levelP, v[1], dec_ds, *k, v[2], v[3], v[4], v[5], B, nullptr, 0, 0, 0, -1, &ks);
    }
    const size_t sQw = (size_t)(levelQ + 1) * N, sPw = (size_t)(levelP + 1) * N;
    TRY(be.ctx->arena_reserve(auto_hoisted_lazy_words(be, levelQ, levelP, B)));
    View t0Q{be.ctx->arena_take(B * sQw), sQw}, t1Q{be.ctx->arena_take(B * sQw), sQw}, t2Q{be.ctx->arena_take(B * sQw), sQw};
    View t0P{be.ctx->arena_take(B * sPw), sPw}, t1P{be.ctx->arena_take(B * sPw), sPw};
    const uint32_t *index = nullptr;
    TRY(cached_auto_index(*ev, gal, &index));
    hipStream_t st = be.ctx->stream;
    TRY(ks_inner(*ev, levelQ, levelP, v[1], dec_ds, *k, t0Q, t0P, t1Q, t1P, B));
    const LimbTab tq = ident_tab(levelQ + 1), tp = ident_tab(levelP + 1, 0, 0, be.LQ);
    // in0 is read before any output is written (c0Q or c1Q may be in0)
    HIP_TRY(launch_ew(be.qp, tq, EW_MUL_SCALAR_MONT, v[0], v[0], t2Q, B, &s, nullptr, st));
    HIP_TRY(launch_ew(be.qp, tq, EW_ADD, t0Q, t2Q, t0Q, B, nullptr, nullptr, st));
    HIP_TRY(launch_gather(be.qp, tq, t1Q, index, v[4], B, false, st));
    HIP_TRY(launch_gather(be.qp, tp, t1P, index, v[5], B, false, st));
    HIP_TRY(launch_gather(be.qp, tq, t0Q, index, v[2], B, false, st));
    HIP_TRY(launch_gather(be.qp, tp, t0P, index, v[3], B, false, st));
    return HE_OK;
}

// The giant step of MultiplyByDiagMatrixBSGS (circuits/common/lintrans/lintrans_evaluator.go:397-441) as one call:
//   (c0, c1) = GadgetProductLazy(levelQ, cx, key);  c0 = ringQP.Add(c0, add);  out_k (+)= AutomorphismNTTWithIndex(c_k)
// (accumulate: ...ThenAddLazy).  On standard rings with the fused decomposition the key inner products store through the
// automorphism themselves (KsScatter giant step: no intermediate ciphertext, no Add and gather passes); otherwise the same
// launches as the separate calls.  Bit-identical to the separate calls either way.
static int giant_step_run(const std::shared_ptr<Evaluator> &ev, const std::shared_ptr<Evk> &k, int levelQ, int levelP, uint64_t gal,
                          int accumulate, const View *v, int B);
int he_lintrans_giant_step(he_handle hev, int levelQ, he_handle hcx, he_handle hk, uint64_t gal, he_handle haddQ, he_handle haddP,
                           he_handle c0Q, he_handle c0P, he_handle c1Q, he_handle c1P, int accumulate) {
    const char *who = "he_lintrans_giant_step";
    GET(ev, Evaluator, hev, T_EVAL);
    GET(k, Evk, hk, T_EVK);
    BasisExtender &be = *ev->be;
    TRY(check_key(*ev, *k, levelQ, who));
    const int levelP = k->nPk - 1;
    if (levelP < 0) return fail(HE_EINVAL, "%s: the key has no special primes", who);
    if (!(gal & 1)) return fail(HE_EINVAL, "%s: Galois element must be odd", who);
    CoReq q;
    Operands o(q, who, be);
    o.in(hcx, levelQ + 1, "cx");
    o.in(haddQ, levelQ + 1, "addQ");
    o.inP(haddP, levelP + 1, "addP");
    o.qp(true, c0Q, c0P, c1Q, c1P, levelQ, levelP);
    TRY(o.check());  // no output may alias an input or another output
    const int B = o.B;
    gal = reduce_gal(gal, be.Q->logN, be.type);
    ks_request(q, CO_GIANT_STEP, ev, k, levelQ, KS_GIANT_STEP, KsAlias{}); q.par[1] = (int64_t)gal; q.par[2] = accumulate ? 1 : 0;
    q.run = [ev, k, levelQ, levelP, gal, accumulate](const View *v, int B) -> int {
        return giant_step_run(ev, k, levelQ, levelP, gal, accumulate, v, B);
    };
    return co_dispatch(*be.ctx, B, q);
}
// the launches of the giant step over B entries: v = (cx, addQ, addP, c0Q, c0P, c1Q, c1P).  The caller holds the context (Scope).
static int giant_step_run(const std::shared_ptr<Evaluator> &ev, const std::shared_ptr<Evk> &k, int levelQ, int levelP, uint64_t gal,
                          int accumulate, const View *v, int B) {
    BasisExtender &be = *ev->be;
    const int N = be.Q->N;
    const bool acc = accumulate != 0;
    // SURVEY 8(d) accounting of the calls this one stands for: GadgetProductLazy + Add on QP + two automorphisms on QP
    be.ctx->acct(levelQ + 1 + 2.0 * (levelQ + levelP + 2) + 3.0 * (levelQ + levelP + 2) + 2.0 * (acc ? 3.0 : 2.0) * (levelQ + levelP + 2),
                 key_limbs(*k, levelQ), B, N);
    { Valu V(be.Q->logN); valu_keyswitch(V, be, levelQ, levelP, base_rns_size(levelQ, levelP), true, true); V.into(*be.ctx, B); }
    const size_t sQw = (size_t)(levelQ + 1) * N, sPw = (size_t)(levelP + 1) * N;
    TRY(be.ctx->arena_reserve(giant_step_words(be, levelQ, levelP, B, k.get())));
    KsCall c;
    TRY(ks_call(*ev, KS_GIANT_STEP, levelQ, *k, KsAlias{}, &c));
    if (c.route.giant_fused) {
        KsScatter ks;
        ks.ginv = galois_inverse(gal, be.Q->logN);
        ks.plain = 1; ks.add0 = v[1]; ks.add0P = v[2]; ks.accumulate = acc ? 1 : 0;
        for (int i = 0; i < kMaxLimbs; i++) ks.add_s[i] = 0;
        LazyArgs a{v[0], B, v[3], v[4], v[5], v[6]};
        a.giant = &ks;
        return gadget_product_lazy_core(*ev, levelQ, *k, c, a);
    }
    // the separate calls' launches
    View t0Q{be.ctx->arena_take(B * sQw), sQw}, t1Q{be.ctx->arena_take(B * sQw), sQw};
    View t0P{be.ctx->arena_take(B * sPw), sPw}, t1P{be.ctx->arena_take(B * sPw), sPw};
    TRY(gadget_product_lazy_core(*ev, levelQ, *k, c, LazyArgs{v[0], B, t0Q, t0P, t1Q, t1P}));
    const uint32_t *index = nullptr;
    TRY(cached_auto_index(*ev, gal, &index));
    hipStream_t st = be.ctx->stream;
    const LimbTab tq = ident_tab(levelQ + 1), tp = ident_tab(levelP + 1, 0, 0, be.LQ);
    HIP_TRY(launch_ew(be.qp, tq, EW_ADD, t0Q, v[1], t0Q, B, nullptr, nullptr, st));
    HIP_TRY(launch_ew(be.qp, tp, EW_ADD, t0P, v[2], t0P, B, nullptr, nullptr, st));
    HIP_TRY(launch_gather(be.qp, tq, t0Q, index, v[3], B, acc, st));
    HIP_TRY(launch_gather(be.qp, tp, t0P, index, v[4], B, acc, st));
    HIP_TRY(launch_gather(be.qp, tq, t1Q, index, v[5], B, acc, st));
    HIP_TRY(launch_gather(be.qp, tp, t1P, index, v[6], B, acc, st));
    return HE_OK;
}

// centred lifts / hoisting-buffer fill of bootstrapping.Evaluator.ModUp (see hering.h)
int he_centered_lift(he_handle hev, int strict, he_handle hsrc, int first_q, int levelQ, he_handle hdq, int levelP, he_handle hdp) {
    GET(ev, Evaluator, hev, T_EVAL);
    BasisExtender &be = *ev->be;
    const char *who = "he_centered_lift";
    if (first_q < 0 || levelQ >= be.LQ || first_q > levelQ + 1 || levelP >= be.LP) return fail(HE_EINVAL, "%s: level out of range", who);
    CoReq q;
    Operands o(q, who, be);
    const int is = o.in(hsrc, 1, "src"), iq = o.out(hdq, levelQ + 1, "dstQ");
    const int ip = o.outP(levelP >= 0 ? o.poly(hdp) : nullptr, levelP + 1, "dstP");
    o.inplace(iq, is);
    TRY(o.check());
    if (levelP < 0) q.ops[ip] = q.ops[iq];  // (no P part: the launch writes nothing through it)
    ModUpArgs a{};
    a.nsrc = 1;
    a.src_limb[0] = 0;
    a.src_mod[0] = 0;
    int n = 0;
    for (int i = first_q; i <= levelQ; i++, n++) { a.dst_limb[n] = (uint8_t)i; a.dst_mod[n] = (uint8_t)i; a.dst_view[n] = 0; }
    for (int j = 0; j <= levelP; j++, n++) { a.dst_limb[n] = (uint8_t)j; a.dst_mod[n] = (uint8_t)(be.LQ + j); a.dst_view[n] = 1; }
    a.ndst = n;
    if (n > kMaxLimbs) return fail(HE_EINVAL, "%s: too many destination limbs", who);
    q.op = CO_CENTERED_LIFT; q.obj = ev.get(); q.par[0] = strict & 3; q.par[1] = first_q; q.par[2] = levelQ; q.par[3] = levelP;
    q.keep.push_back(ev);
    q.run = [ev, a, n, strict](const View *v, int B) -> int {
        BasisExtender &be = *ev->be;
        be.ctx->acct(1.0 + n, 0, B, be.Q->N);
        HIP_TRY(launch_center_copy(be.qp, a, v[0], v[1], v[2], B, be.ctx->stream, strict & 3));
        return HE_OK;
    };
    return co_dispatch(*be.ctx, o.B, q);
}
int he_decomp_fill(he_handle hdec, int levelQ, int levelP, he_handle hq, he_handle hp) {
    GET(d, Decomp, hdec, T_DECOMP);
    BasisExtender &be = *d->ev->be;
    const char *who = "he_decomp_fill";
    if (levelQ < 0 || levelQ >= be.LQ || levelP < 0 || levelP >= be.LP) return fail(HE_EINVAL, "%s: level out of range", who);
    CoReq q;
    Operands o(q, who, be, d->batch);
    o.in(hq, levelQ + 1, "srcQ");
    o.inP(hp, levelP + 1, "srcP");
    o.raw(d->view(), d);
    TRY(o.check());
    d->fillQ = -1;  // see he_decompose_ntt
    const std::shared_ptr<Evaluator> ev = d->ev;
    const int beta_max = d->beta_max;
    const size_t dec_ds = d->dstride();
    q.op = CO_DECOMP_FILL; q.obj = ev.get(); q.par[0] = levelQ; q.par[1] = levelP;
    q.keep.push_back(ev);
    q.run = [ev, levelQ, levelP, beta_max, dec_ds](const View *v, int B) -> int {
        BasisExtender &be = *ev->be;
        be.ctx->acct(levelQ + levelP + 2 + (double)beta_max * (levelQ + levelP + 2), 0, B, be.Q->N);
        for (int dg = 0; dg < beta_max; dg++) {  // every digit block takes a copy of the Q part and of the P part
            View blk{v[2].p + (size_t)dg * dec_ds, v[2].bstride, v[2].tab};
            HIP_TRY(launch_ew(be.qp, ident_tab(levelQ + 1), EW_COPY, v[0], v[0], blk, B, nullptr, nullptr, be.ctx->stream));
            HIP_TRY(launch_ew(be.qp, ident_tab(levelP + 1, 0, be.LQ, be.LQ), EW_COPY, v[1], v[1], blk, B, nullptr, nullptr, be.ctx->stream));
        }
        return HE_OK;
    };
    TRY(co_dispatch(*be.ctx, d->batch, q));
    d->fillQ = levelQ; d->fillP = levelP; d->fill_beta = d->beta_max;
    return HE_OK;
}

// inner accumulation of the lintrans drivers (see hering.h)
int he_lintrans_mul_sum(he_handle hev, int levelQ, int levelP, int n, const he_handle *ptQ, const he_handle *ptP,
                        const he_handle *ct0Q, const he_handle *ct0P, const he_handle *ct1Q, const he_handle *ct1P,
                        const he_handle *index, int accumulate, he_handle o0Q, he_handle o0P, he_handle o1Q, he_handle o1P) {
    GET(ev, Evaluator, hev, T_EVAL);
    BasisExtender &be = *ev->be;
    const char *who = "he_lintrans_mul_sum";
    if (n < 0 || n > kMaxDiag) return fail(HE_EINVAL, "%s: n must be in [0, %d]", who, kMaxDiag);
    if (levelQ < 0 || levelQ >= be.LQ || levelP < 0 || levelP >= be.LP) return fail(HE_EINVAL, "%s: level out of range", who);
    if (n > 0 && (!ptQ || !ptP || !ct0Q || !ct0P || !ct1Q || !ct1P)) return fail(HE_EINVAL, "%s: null array", who);
    // operands of the request: [0..3] the outputs, then per term i: 6 i + 4 + {0: ptQ, 1: c0Q, 2: c1Q, 3: ptP, 4: c0P, 5: c1P}
    // (null views for the P part of a term without one)
    CoReq q;
    q.op = CO_LINTRANS; q.obj = ev.get(); q.par[0] = levelQ; q.par[1] = levelP; q.par[2] = n; q.par[3] = accumulate ? 1 : 0;
    Operands o(q, who, be);
    o.qp(true, o0Q, o0P, o1Q, o1P, levelQ, levelP);
    q.keep.push_back(ev);
    std::vector<const uint32_t *> idx(n, nullptr);
    std::vector<uint64_t> idx_gal(n, 0);
    for (int i = 0; i < n; i++) {
        if (index && index[i]) {
            GET(ixo, AutoIndex, index[i], T_INDEX);
            if (ixo->N != be.Q->N) return fail(HE_EINVAL, "%s: automorphism index of another degree", who);
            idx[i] = ixo->d;
            idx_gal[i] = ixo->gal;
            q.keep.push_back(ixo);
        }
        q.blob.push_back(idx_gal[i]);  // (the rotation of the term is part of the key -- by Galois element, see gather_api)
        q.blob.push_back((uint64_t)(uintptr_t)idx[i]);  // ... and by the cached table (another ring type: another permutation)
        if ((ct0P[i] == 0) != (ct1P[i] == 0)) return fail(HE_EINVAL, "%s: term %d has only one P part", who, i);
        const bool hasP = ct0P[i] != 0;
        o.in(ptQ[i], levelQ + 1, "ptQ", Operands::kBroadcast);  // one plaintext diagonal may serve the whole batch
        o.in(ct0Q[i], levelQ + 1, "ct0Q");
        o.in(ct1Q[i], levelQ + 1, "ct1Q");
        o.inP(hasP ? o.poly(ptP[i]) : nullptr, levelP + 1, "ptP", Operands::kBroadcast);
        o.inP(hasP ? o.poly(ct0P[i]) : nullptr, levelP + 1, "ct0P");
        o.inP(hasP ? o.poly(ct1P[i]) : nullptr, levelP + 1, "ct1P");
    }
    TRY(o.check());  // the outputs alias nothing: the terms' inputs are read by every workgroup of both launches
    q.run = [ev, levelQ, levelP, n, accumulate, idx](const View *v, int B) -> int {
        BasisExtender &be = *ev->be;
        DiagMacArgs aq{}, ap{};
        aq.n = ap.n = n;
        aq.nlimbs = levelQ + 1; ap.nlimbs = levelP + 1;
        aq.accumulate = ap.accumulate = accumulate ? 1 : 0;
        aq.mod0 = 0; ap.mod0 = be.LQ;
        const bool tabs = v[0].tab != nullptr;  // a coalesced batch: the terms' operands are rows 4 + 6 i ... of the entry table
        double per = 2.0, shared = 0.0;
        for (int i = 0; i < n; i++) {
            const View *t = v + 4 + 6 * i;
            aq.pt[i] = t[0].p; aq.pt_bs[i] = t[0].bstride;
            aq.c0[i] = t[1].p; aq.c0_bs[i] = t[1].bstride;
            aq.c1[i] = t[2].p; aq.c1_bs[i] = t[2].bstride;
            ap.pt[i] = t[3].p; ap.pt_bs[i] = t[3].bstride;
            ap.c0[i] = t[4].p; ap.c0_bs[i] = t[4].bstride;
            ap.c1[i] = t[5].p; ap.c1_bs[i] = t[5].bstride;
            aq.index[i] = ap.index[i] = idx[i];
            // per term: the plaintext diagonal (shared by the batch when it has batch 1) and both ciphertext components
            per += 2.0;
            if (t[0].bstride || tabs) per += 1.0; else shared += 1.0;
        }
        if (tabs && n > 0) {  // (n == 0: the request has four operands only)
            // rows 4 + 6 i + {0, 1, 2} are the Q part's (pt, c0, c1) of term i, + {3, 4, 5} the P part's: DiagMacArgs::term_tab wants
            // [3 i + j][B] -- a table with a stride of six rows per term, so the Q launch starts at row 4, the P launch at row 7,
            // and both skip the other part's three rows (term_tab_rows = 6)
            aq.term_tab = v[4].tab; ap.term_tab = v[4].tab + (size_t)3 * B;
            aq.term_rows = ap.term_rows = 6;
        }
        be.ctx->acct(per * (levelQ + levelP + 2), shared * (levelQ + levelP + 2), B, be.Q->N);
        { Valu V(be.Q->logN); for (int i = 0; i <= levelQ; i++) V.mul(cls_f64(be.small, i), 2.0 * n + 2.0); for (int j = 0; j <= levelP; j++) V.mul(cls_f64(be.small, be.LQ + j), 2.0 * n + 2.0); V.into(*be.ctx, B); }
        hipStream_t st = be.ctx->stream;
        HIP_TRY(launch_diag_mac(be.qp, aq, v[0], v[2], B, st));
        HIP_TRY(launch_diag_mac(be.qp, ap, v[1], v[3], B, st));
        return HE_OK;
    };
    return co_dispatch(*be.ctx, o.B, q);
}

// CKKS mulRelin / BGV tensorStandard (schemes/ckks/evaluator.go:764-872, schemes/bgv/evaluator.go:592-685)
// The launches of one call over B entries; the caller holds the context (Scope).  `alias`: some output is an input of its own
// entry.  The views may carry entry tables (a coalesced batch) when the route said so.
static int mul_relin_core(Evaluator &ev, int level, bool bgv, uint64_t t, Evk *k, View a0, View a1, View b0, View b1, View o0v, View o1v,
                          View o2v, int B, KsAlias alias) {
    BasisExtender &be = *ev.be;
    std::vector<uint64_t> sc_(level + 1);
    for (int i = 0; i <= level; i++) {
        const ModConst &m = be.Q->sub[i].mc;
        if (bgv) {  // tMontgomery = MForm(t * 2^64 mod q)                     schemes/bgv/evaluator.go:59-62
            const uint64_t w[2] = {0, t};
            sc_[i] = mform(words_mod(w, 2, m.q), m.q, m.brc0, m.brc1);
        } else {    // MForm(x) = MRed(x, 2^128 mod q)
            sc_[i] = m.r2;
        }
    }
    const int N = be.Q->N;
    {
        Valu V(be.Q->logN);
        for (int i = 0; i <= level; i++) V.mul(cls_f64(be.small, i), 6.0);  // the tensor
        if (k) valu_gadget_product(V, be, level, k->nPk - 1, key_beta(*k, level), true);
        V.into(*be.ctx, B);
    }
    if (k) be.ctx->acct(6.0 * (level + 1), key_limbs(*k, std::min(level, k->nQk - 1)), B, N);  // MulRelin: 6 L + 2 beta (L + alpha)
    else be.ctx->acct(7.0 * (level + 1), 0, B, N);                                                // Mul: 4 L in, 3 L out
    const size_t wQ = (size_t)B * (level + 1) * N;
    hipStream_t st = be.ctx->stream;
    if (!k) {
        HIP_TRY(launch_tensor(be.qp, ident_tab(level + 1), sc_.data(), a0, a1, b0, b1, o0v, o1v, o2v, B, st));
        return HE_OK;
    }
    TRY(be.ctx->arena_reserve(ks_scratch_words(be, level, k->nPk - 1, B, true, k) + wQ));
    View c2{be.ctx->arena_take(wQ), (size_t)(level + 1) * N};
    KsCall c;
    TRY(ks_call(ev, KS_MUL_RELIN, level, *k, alias, &c));
    GpArgs g{&c2, nullptr, o0v, o1v, B, nullptr, nullptr, true};  // c2 is formed here: canonical
    // With the tensor terms in the ModDown epilogue the tensor kernel forms c2 only, and that on the way: by the inverse row pass
    // for the double-precision limbs, by the tensor kernel for the others (24 limbs of writes and 24 of reads fewer; the inputs'
    // second read comes from L2).
    const TensorIn tin{a0, a1, b0, b1, sc_.data()};
    if (c.route.tensor_epilogue) g.tin = &tin;
    else {
        HIP_TRY(launch_tensor(be.qp, ident_tab(level + 1), sc_.data(), a0, a1, b0, b1, o0v, o1v, c2, B, st));
        g.add0 = &o0v; g.add1 = &o1v;
    }
    return gadget_product_core(ev, level, *k, c, g);
}

static int mul_relin_common(he_handle hev, int level, bool bgv, uint64_t t, he_handle ha0, he_handle ha1, he_handle hb0, he_handle hb1,
                            he_handle hk, he_handle hout0, he_handle hout1, he_handle hout2, const char *who) {
    GET(ev, Evaluator, hev, T_EVAL);
    std::shared_ptr<Evk> k;
    BasisExtender &be = *ev->be;
    if (level < 0 || level >= be.LQ) return fail(HE_EINVAL, "%s: level out of range", who);
    if (hk) {
        k = get<Evk>(hk, T_EVK);
        if (!k) return fail(HE_EHANDLE, "%s: bad relinearization key handle", who);
        int lv = level;
        TRY(check_key(*ev, *k, lv, who));
        if (lv != level) return fail(HE_EINVAL, "%s: relinearization key level %d below ciphertext level %d", who, k->nQk - 1, level);
    }
    CoReq q;
    Operands o(q, who, be);
    const int i0 = o.in(ha0, level + 1, "a0");
    o.in(ha1, level + 1, "a1");
    o.in(hb0, level + 1, "b0");
    o.in(hb1, level + 1, "b1");
    const int o0 = o.out(hout0, level + 1, "out0"), o1 = o.out(hout1, level + 1, "out1");
    o.out(k ? nullptr : o.poly(hout2), level + 1, "out2 (required when no relinearization key is given)");  // an output only without a key
    o.all_inplace = true;  // any output may be any input (MulRelin(res, res, res))
    TRY(o.check());
    KsAlias alias;
    for (int in = i0; in < i0 + 4; in++) alias.out_is_addend = alias.out_is_addend || o.same(o0, in) || o.same(o1, in);
    // (a degree-2 output that is one of the inputs: the tensor kernel reads all four inputs of a coefficient before it writes)
    ks_request(q, k ? CO_MUL_RELIN : CO_MUL, ev, k, level, KS_MUL_RELIN, alias); q.par[1] = bgv; q.par[2] = (int64_t)(bgv ? t : 0);
    q.run = [ev, k, level, bgv, t, alias](const View *v, int B) -> int {
        return mul_relin_core(*ev, level, bgv, t, k.get(), v[0], v[1], v[2], v[3], v[4], v[5], v[6], B, alias);
    };
    return co_dispatch(*be.ctx, o.B, q);
}
int he_ckks_mul_relin(he_handle ev, int level, he_handle a0, he_handle a1, he_handle b0, he_handle b1, he_handle rlk, he_handle o0, he_handle o1, he_handle o2) {
    return mul_relin_common(ev, level, false, 0, a0, a1, b0, b1, rlk, o0, o1, o2, "he_ckks_mul_relin");
}
int he_bgv_mul_relin(he_handle ev, int level, uint64_t t, he_handle a0, he_handle a1, he_handle b0, he_handle b1, he_handle rlk, he_handle o0, he_handle o1, he_handle o2) {
    return mul_relin_common(ev, level, true, t, a0, a1, b0, b1, rlk, o0, o1, o2, "he_bgv_mul_relin");
}

// ---------------------------------------------------------------------------------------
// ckks.Evaluator (include/hering_ckks_evaluator.h; schemes/ckks/evaluator.go): the linear forms over a whole ciphertext and
// MulRelinThenAdd, one queued request and one launch of ct_lin_kernel / tensor_add_kernel each
// ---------------------------------------------------------------------------------------
// the residues of an integer on the limbs 0 .. level, each below its modulus: as they are, or in Montgomery form
static int ckks_words(const Ring &r, int level, const uint64_t *w, bool mont, uint64_t *out, const char *who, const char *name) {
    for (int i = 0; i <= level; i++) {
        const ModConst &m = r.sub[i].mc;
        if (w[i] >= m.q) return fail(HE_EINVAL, "%s: %s[%d] is not below its modulus", who, name, i);
        out[i] = mont ? mform(w[i], m.q, m.brc0, m.brc1) : w[i];
    }
    return HE_OK;
}
static int ckks_list(const char *who, const char *name, int n, const he_handle *h) {
    if (n < 1 || n > 3 || !h) return fail(HE_EINVAL, "%s: %s must hold 1 to 3 components", who, name);
    return HE_OK;
}
// files the request of one ct_lin_kernel launch: the operands were declared x (n_x of them), y (a.ny), z (n_x or a.nz) in this
// order; a.nx / a.nz may be smaller than the declared lists (the scalar Add / Sub in place moves no other component)
static int ct_lin_file(const std::shared_ptr<Ring> &r, int level, CoReq &q, const CtLinArgs &a, int n_x, int n_z, int B) {
    q.op = CO_CT_LIN; q.obj = r.get(); q.par[0] = level; q.par[1] = a.form; q.par[2] = a.scaled;
    q.par[3] = a.nx | (a.ny << 4) | (a.nz << 8); q.par[4] = n_x | (n_z << 4);
    q.blob.assign(a.r, a.r + level + 1);
    q.blob.insert(q.blob.end(), a.s, a.s + level + 1);
    q.blob.insert(q.blob.end(), a.s2, a.s2 + level + 1);
    q.keep.push_back(r);
    q.run = [r, level, a, n_x](const View *v, int B) -> int {
        CtLinArgs k = a;
        double shared = 0.0;  // a batch-1 operand is read once for the whole batch
        for (int i = 0; i < k.nx; i++) k.x[i] = v[i];
        for (int i = 0; i < k.ny; i++) { k.y[i] = v[n_x + i]; shared += (double)(k.y[i].bstride == 0 && !k.y[i].tab && B > 1); }
        for (int i = 0; i < k.nz; i++) k.z[i] = v[n_x + a.ny + i];
        r->ctx->acct((ct_lin_passes(k) - shared) * (level + 1), shared * (level + 1), B, r->N);
        const bool acc = k.form == CT_SCALAR_MUL_ADD || k.form == CT_PT_MUL_ADD;
        double muls = 0.0;  // modular products per coefficient of a limb
        if (k.form == CT_ADD || k.form == CT_SUB) muls = k.scaled == 1 ? k.nx : (k.scaled == 2 ? k.ny : 0);
        else if (k.form != CT_SCALAR_ADD && k.form != CT_SCALAR_SUB)
            muls = k.nx + ((k.form == CT_PT_MUL || k.form == CT_PT_MUL_ADD) ? 1 : 0) + (acc && k.scaled ? k.nz : 0);
        if (muls > 0) { Valu V(r->logN); for (int i = 0; i <= level; i++) V.mul(cls_f64(r->small, i), muls); V.into(*r->ctx, B); }
        HIP_TRY(launch_ct_lin(r->dev, k, B, r->ctx->stream));
        return HE_OK;
    };
    return co_dispatch(*r->ctx, B, q);
}
int he_ckks_add(he_handle hring, int level, int sub, int n0, const he_handle *op0, int n1, const he_handle *op1, int scaled,
                const uint64_t *ratio, int n_out, const he_handle *out) {
    GET(r, Ring, hring, T_RING);
    const char *who = "he_ckks_add";
    TRY(check_level(*r, level, who));
    TRY(ckks_list(who, "op0", n0, op0));
    TRY(ckks_list(who, "op1", n1, op1));
    TRY(ckks_list(who, "out", n_out, out));
    if (n_out != std::max(n0, n1)) return fail(HE_EINVAL, "%s: out has %d components, max(%d, %d) expected", who, n_out, n0, n1);
    if ((sub != 0 && sub != 1) || scaled < 0 || scaled > 2 || (scaled && !ratio)) return fail(HE_EINVAL, "%s: bad arguments", who);
    if (r->N < 4) return fail(HE_EINVAL, "%s: ring degree %d, at least 4 needed", who, r->N);
    CtLinArgs a{};
    a.form = sub ? CT_SUB : CT_ADD; a.scaled = scaled; a.nx = n0; a.ny = n1; a.nz = n_out; a.nlimbs = level + 1;
    if (scaled) TRY(ckks_words(*r, level, ratio, true, a.r, who, "ratio"));
    CoReq q;
    Operands o(q, who, *r);
    for (int i = 0; i < n0; i++) o.in(op0[i], level + 1, "op0");
    for (int i = 0; i < n1; i++) o.in(op1[i], level + 1, "op1", Operands::kBroadcast);
    for (int i = 0; i < n_out; i++) o.out(out[i], level + 1, "out");
    o.all_inplace = true;  // any output may be any input: a thread reads every input word of its coefficients before it writes
    TRY(o.check());
    return ct_lin_file(r, level, q, a, n0, n_out, o.B);
}
int he_ckks_scalar(he_handle hring, int level, int op, int n, const he_handle *op0, const uint64_t *s0, const uint64_t *s1,
                   const uint64_t *pre, const he_handle *out) {
    GET(r, Ring, hring, T_RING);
    const char *who = "he_ckks_scalar";
    TRY(check_level(*r, level, who));
    TRY(ckks_list(who, "op0", n, op0));
    TRY(ckks_list(who, "out", n, out));
    if (op < HE_CKKS_SCALAR_ADD || op > HE_CKKS_SCALAR_MUL_THEN_ADD || !s0 || !s1) return fail(HE_EINVAL, "%s: bad arguments", who);
    if (pre && op != HE_CKKS_SCALAR_MUL_THEN_ADD) return fail(HE_EINVAL, "%s: pre is taken by HE_CKKS_SCALAR_MUL_THEN_ADD only", who);
    if (r->N < 4) return fail(HE_EINVAL, "%s: ring degree %d, at least 4 needed", who, r->N);
    static const int forms[4] = {CT_SCALAR_ADD, CT_SCALAR_SUB, CT_SCALAR_MUL, CT_SCALAR_MUL_ADD};
    CtLinArgs a{};
    a.form = forms[op]; a.scaled = pre ? 1 : 0; a.nx = a.nz = n; a.ny = 0; a.nlimbs = level + 1;
    const bool mont = op >= HE_CKKS_SCALAR_MUL;  // MulDoubleRNSScalar takes MForm of the scalars (ring/operations.go:249-268)
    TRY(ckks_words(*r, level, s0, mont, a.s, who, "s0"));
    TRY(ckks_words(*r, level, s1, mont, a.s2, who, "s1"));
    if (pre) TRY(ckks_words(*r, level, pre, true, a.r, who, "pre"));
    CoReq q;
    Operands o(q, who, *r);
    for (int i = 0; i < n; i++) o.in(op0[i], level + 1, "op0");
    for (int i = 0; i < n; i++) o.out(out[i], level + 1, "out");
    o.all_inplace = true;
    TRY(o.check());
    if (op <= HE_CKKS_SCALAR_SUB) {  // in place (:82-86): the components past the first stay where they are
        bool same = true;
        for (int i = 1; i < n; i++) same = same && o.same(i, n + i);
        if (same) a.nx = a.nz = 1;
    }
    return ct_lin_file(r, level, q, a, n, n, o.B);
}
int he_ckks_mul_pt(he_handle hring, int level, int n, const he_handle *ct, he_handle pt, int then_add, const uint64_t *pre,
                   const he_handle *out) {
    GET(r, Ring, hring, T_RING);
    const char *who = "he_ckks_mul_pt";
    TRY(check_level(*r, level, who));
    TRY(ckks_list(who, "ct", n, ct));
    TRY(ckks_list(who, "out", n, out));
    if (then_add != 0 && then_add != 1) return fail(HE_EINVAL, "%s: bad arguments", who);
    if (pre && !then_add) return fail(HE_EINVAL, "%s: pre is taken with then_add only", who);
    if (r->N < 4) return fail(HE_EINVAL, "%s: ring degree %d, at least 4 needed", who, r->N);
    CtLinArgs a{};
    a.form = then_add ? CT_PT_MUL_ADD : CT_PT_MUL; a.scaled = pre ? 1 : 0; a.nx = a.nz = n; a.ny = 1; a.nlimbs = level + 1;
    if (pre) TRY(ckks_words(*r, level, pre, true, a.r, who, "pre"));
    CoReq q;
    Operands o(q, who, *r);
    for (int i = 0; i < n; i++) o.in(ct[i], level + 1, "ct");
    o.in(pt, level + 1, "pt", Operands::kBroadcast);
    for (int i = 0; i < n; i++) o.out(out[i], level + 1, "out");
    o.all_inplace = true;
    TRY(o.check());
    return ct_lin_file(r, level, q, a, n, n, o.B);
}
int he_ckks_mul_relin_then_add(he_handle hev, int level, he_handle ha0, he_handle ha1, he_handle hb0, he_handle hb1, he_handle hk,
                               const uint64_t *pre, he_handle hout0, he_handle hout1, he_handle hout2) {
    GET(ev, Evaluator, hev, T_EVAL);
    const char *who = "he_ckks_mul_relin_then_add";
    std::shared_ptr<Evk> k;
    BasisExtender &be = *ev->be;
    if (level < 0 || level >= be.LQ) return fail(HE_EINVAL, "%s: level out of range", who);
    if (be.Q->N < 4) return fail(HE_EINVAL, "%s: ring degree %d, at least 4 needed", who, be.Q->N);
    if (hk) {
        k = get<Evk>(hk, T_EVK);
        if (!k) return fail(HE_EHANDLE, "%s: bad relinearization key handle", who);
        int lv = level;
        TRY(check_key(*ev, *k, lv, who));
        if (lv != level) return fail(HE_EINVAL, "%s: relinearization key level %d below ciphertext level %d", who, k->nQk - 1, level);
        if (hout2) return fail(HE_EINVAL, "%s: out2 must be 0 when a relinearization key is given", who);
    }
    TensorAddArgs t{};
    t.nlimbs = level + 1; t.has_r = pre ? 1 : 0;
    if (pre) TRY(ckks_words(*be.Q, level, pre, true, t.r, who, "pre"));
    CoReq q;
    Operands o(q, who, be);
    o.in(ha0, level + 1, "a0");
    o.in(ha1, level + 1, "a1");
    o.in(hb0, level + 1, "b0");
    o.in(hb1, level + 1, "b1");
    o.out(hout0, level + 1, "out0");
    o.out(hout1, level + 1, "out1");
    o.out(k ? nullptr : o.poly(hout2), level + 1, "out2 (required when no relinearization key is given)");
    TRY(o.check());  // (no in-place form: an output that is an input is the reference's error, evaluator.go:918, :1064)
    if (!k && !q.ops[6].p) return fail(HE_EINVAL, "%s: out2 is required when no relinearization key is given", who);
    ks_request(q, CO_TENSOR_ADD, ev, k, level, KS_GADGET_PRODUCT, KsAlias{});
    q.par[1] = t.has_r;
    q.blob.assign(t.r, t.r + level + 1);
    q.run = [ev, k, level, t](const View *v, int B) -> int {
        BasisExtender &be = *ev->be;
        const int N = be.Q->N;
        TensorAddArgs a = t;
        a.a0 = v[0]; a.a1 = v[1]; a.b0 = v[2]; a.b1 = v[3]; a.acc0 = a.c0 = v[4]; a.acc1 = a.c1 = v[5];
        {
            Valu V(be.Q->logN);
            for (int i = 0; i <= level; i++) V.mul(cls_f64(be.small, i), 6.0 + (a.has_r ? (k ? 2.0 : 3.0) : 0.0));
            V.into(*be.ctx, B);
        }
        be.ctx->acct((k ? 9.0 : 10.0) * (level + 1), 0, B, N);  // four inputs, the accumulators in, three outputs
        if (!k) {
            a.acc2 = a.c2 = v[6];
            HIP_TRY(launch_tensor_add(be.qp, a, B, be.ctx->stream));
            return HE_OK;
        }
        // with a key: c2 to scratch, then the gadget product with the accumulated (c0, c1) as the ModDown epilogue's addends --
        // he_relinearize in place on (out0, out1)
        const size_t wQ = (size_t)B * (level + 1) * N;
        TRY(keyswitch_begin(*ev, *k, level, 5.0 * (level + 1), true, B, wQ + 4));
        View c2{be.ctx->arena_take(wQ), (size_t)(level + 1) * N};
        a.acc2 = View{nullptr, 0}; a.c2 = c2;
        HIP_TRY(launch_tensor_add(be.qp, a, B, be.ctx->stream));
        GpArgs g{&c2, nullptr, v[4], v[5], B, &v[4], &v[5]};
        g.cx_canonical = true;  // c2 is formed here
        return key_switch(*ev, KS_GADGET_PRODUCT, level, *k, KsAlias{}, g);
    };
    return co_dispatch(*be.ctx, o.B, q);
}

// ---------------------------------------------------------------------------------------
// BFV: the scale-invariant multiplication (include/hering_bfv.h; schemes/bgv/evaluator.go:38-70, :898-1071)
// ---------------------------------------------------------------------------------------
// evaluatorBase (evaluator.go:31-36) beside a device evaluator: the basis extender Q <-> QMul, levelQMul and t in Montgomery form
struct BfvEvaluator : Obj {
    std::shared_ptr<Evaluator> ev;
    std::shared_ptr<BasisExtender> be;  // basisExtenderQ1toQ2: Q = the evaluator's RingQ, P = ringQMul
    uint64_t t = 0;
    std::vector<int> level_qmul;        // by level of Q
    std::vector<uint64_t> t_mont;       // MForm(t mod q_i): the scalar of ringQ.MulScalar (ring/operations.go:201)
    BfvEvaluator() : Obj(T_BFV) {}
};
// bits of prod(m[0..n)) (big.Int.BitLen of evaluator.go:46-47)
static std::vector<int> product_bitlens(const std::vector<uint64_t> &m) {
    std::vector<uint64_t> w{1};
    std::vector<int> out;
    for (uint64_t q : m) {
        uint64_t carry = 0;
        for (uint64_t &x : w) {
            const u128 p = (u128)x * q + carry;
            x = (uint64_t)p; carry = (uint64_t)(p >> 64);
        }
        if (carry) w.push_back(carry);
        out.push_back((int)(w.size() - 1) * 64 + (64 - __builtin_clzll(w.back())));
    }
    return out;
}
int he_bfv_evaluator_create(he_handle hev, he_handle hqmul, uint64_t t, he_handle *out) {
    static const char *who = "he_bfv_evaluator_create";
    GET(ev, Evaluator, hev, T_EVAL);
    GET(M, Ring, hqmul, T_RING);
    if (!out) return fail(HE_EINVAL, "%s: null output", who);
    const std::shared_ptr<Ring> Q = ev->be->Q;
    if (t == 0) return fail(HE_EINVAL, "%s: the plaintext modulus is zero", who);
    if (M->ctx != Q->ctx) return fail(HE_EINVAL, "%s: ringQMul belongs to another context", who);
    if (M->N != Q->N) return fail(HE_EINVAL, "%s: ringQMul has degree %d, the evaluator's ring %d", who, M->N, Q->N);
    if (Q->type != 0 || M->type != 0)
        return fail(HE_EINVAL, "%s: conjugate-invariant rings are not served (%s); bgv parameters are standard", who, Q->type ? "the evaluator" : "ringQMul");
    if (Q->nmod() > 32 || M->nmod() > 32)
        return fail(HE_EINVAL, "%s: %d moduli in Q and %d in QMul, at most 32 each (ring/basis_extension.go:285)", who, Q->nmod(), M->nmod());
    auto b = std::make_shared<BfvEvaluator>();
    b->ev = ev; b->t = t;
    for (int bits : product_bitlens(Q->moduli)) b->level_qmul.push_back((bits + Q->logN + 60) / 61 - 1);  // evaluator.go:47
    if (b->level_qmul.back() > M->nmod() - 1)
        return fail(HE_EINVAL, "%s: ringQMul has %d moduli, levelQMul at the top level is %d", who, M->nmod(), b->level_qmul.back());
    he_handle hbe = 0;
    TRY(basis_extender_build(Q, M, &hbe));
    b->be = get<BasisExtender>(hbe, T_BE);
    reg_drop(hbe);  // owned by this object
    for (const SubRingHost &sr : Q->sub) b->t_mont.push_back(mform(t, sr.mc.q, sr.mc.brc0, sr.mc.brc1));
    *out = reg(b);
    return HE_OK;
}
int he_bfv_evaluator_destroy(he_handle h) { return unreg(h, T_BFV); }
int he_bfv_level_qmul(he_handle h, int level, int *lm) {
    GET(b, BfvEvaluator, h, T_BFV);
    if (!lm) return fail(HE_EINVAL, "he_bfv_level_qmul: null output");
    TRY(check_level(*b->be->Q, level, "he_bfv_level_qmul"));
    *lm = b->level_qmul[level];
    return HE_OK;
}
// the middle of quantize (:1057-1067) over `nb` coefficient-domain entries: cQ (level + 1 limbs) and cM (lm + 1 limbs) -> out
static int bfv_quantize_launch(const BfvEvaluator &b, int level, View cQ, View cM, View outQ, int nb) {
    const BasisExtender &be = *b.be;
    const int lm = b.level_qmul[level];
    const std::vector<uint64_t> Qb(be.Q->moduli.begin(), be.Q->moduli.begin() + level + 1), Mb(be.P->moduli.begin(), be.P->moduli.begin() + lm + 1);
    BfvQuantizeArgs a{};
    a.nq = level + 1; a.nm = lm + 1; a.mod_m0 = be.LQ;
    for (int i = 0; i <= level; i++) {
        a.q_half_q[i] = half_product_mod(Qb, Qb[i]);
        a.m_half_q[i] = half_product_mod(Mb, Qb[i]);
        a.t_mont[i] = b.t_mont[i];
    }
    for (int j = 0; j <= lm; j++) {
        a.q_half_m[j] = half_product_mod(Qb, Mb[j]);
        a.m_half_m[j] = half_product_mod(Mb, Mb[j]);
        a.div_s[j] = Mb[j] - be.md_qtop[level][j];
    }
    HIP_TRY(launch_bfv_quantize(be.qp, be.qtop[level].on(be.pool), be.ptoq[lm].on(be.pool), a, cQ, cM, outQ, nb, be.ctx->stream));
    return HE_OK;
}
// bytes and arithmetic of the quantize of one polynomial between its transforms: 2 (L + lm) limbs, two reconstructions
static void bfv_quantize_acct(const BfvEvaluator &b, int level, int lm, Valu &V) {
    const BasisExtender &be = *b.be;
    std::vector<int> dq, dm;
    for (int i = 0; i <= level; i++) { dq.push_back(i); V.mul(false, 1.0); }
    for (int j = 0; j <= lm; j++) { dm.push_back(be.LQ + j); V.mul(false, 1.0); }
    valu_modup(V, be.small, 0, level + 1, dm);
    valu_modup(V, be.small, be.LQ, lm + 1, dq);
}
int he_bfv_quantize(he_handle hb, int level, he_handle hcq, he_handle hcm, he_handle hout) {
    static const char *who = "he_bfv_quantize";
    GET(b, BfvEvaluator, hb, T_BFV);
    BasisExtender &be = *b->be;
    TRY(check_level(*be.Q, level, who));
    const int lm = b->level_qmul[level];
    CoReq q;
    Operands o(q, who, be);
    const int iq = o.in(hcq, level + 1, "cQ");
    o.inP(hcm, lm + 1, "cM");
    o.inplace(o.out(hout, level + 1, "outQ"), iq);
    TRY(o.check());
    if (o.B > 65535) return fail(HE_EINVAL, "%s: %d entries in one call, at most 65535 (split the batch)", who, o.B);
    q.op = CO_BFV_QUANTIZE; q.obj = b.get(); q.par[0] = level;
    q.keep.push_back(b);
    q.run = [b, level, lm](const View *v, int B) -> int {
        BasisExtender &be = *b->be;
        const int N = be.Q->N;
        const size_t sQ = (size_t)(level + 1) * N, sM = (size_t)(lm + 1) * N;
        be.ctx->acct(2.0 * (level + 1) + lm + 1, 0, B, N);
        {
            Valu V(be.Q->logN);
            for (int i = 0; i <= level; i++) V.ntt(cls_f64(be.small, i), 2.0);
            for (int j = 0; j <= lm; j++) V.ntt(cls_f64(be.small, be.LQ + j));
            bfv_quantize_acct(*b, level, lm, V);
            V.into(*be.ctx, B);
        }
        TRY(be.ctx->arena_reserve(B * (sQ + sM) + 4));
        const View tQ{be.ctx->arena_take(B * sQ), sQ}, tM{be.ctx->arena_take(B * sM), sM};
        HIP_TRY(be_ntt(be, ident_tab(level + 1), v[0], tQ, B, true, NTT_REDUCE_INPUT));
        HIP_TRY(be_ntt(be, ident_tab(lm + 1, 0, 0, be.LQ), v[1], tM, B, true, NTT_REDUCE_INPUT));
        TRY(bfv_quantize_launch(*b, level, tQ, tM, tQ, B));
        HIP_TRY(be_ntt(be, ident_tab(level + 1), tQ, v[2], B, false, NTT_REDUCE_INPUT));
        return HE_OK;
    };
    q.one_by_one();  // (the quantize launch takes no entry tables)
    return co_dispatch(*be.ctx, o.B, q);
}
// tensorScaleInvariant (:898-972).  Everything between the inputs and the outputs lives in scratch: the inverse transforms of the
// nin = 4 (squaring: 2) input components [nin][B], their extension to QMul [nin][B], the products on Q and on QMul [3][B].  The
// inputs are last read by the Q tensor, the first output word is written by the final transform (or the key switch's epilogue):
// any output may be any input.
int he_bfv_mul_relin(he_handle hb, int level, he_handle ha0, he_handle ha1, he_handle hb0, he_handle hb1, he_handle hk, he_handle hout0,
                     he_handle hout1, he_handle hout2) {
    static const char *who = "he_bfv_mul_relin";
    GET(b, BfvEvaluator, hb, T_BFV);
    const std::shared_ptr<Evaluator> ev = b->ev;
    BasisExtender &be = *b->be;
    TRY(check_level(*be.Q, level, who));
    std::shared_ptr<Evk> k;
    if (hk) {
        k = get<Evk>(hk, T_EVK);
        if (!k) return fail(HE_EHANDLE, "%s: bad relinearization key handle", who);
        int lv = level;
        TRY(check_key(*ev, *k, lv, who));
        if (lv != level) return fail(HE_EINVAL, "%s: relinearization key level %d below ciphertext level %d", who, k->nQk - 1, level);
    }
    const bool square = ha0 == hb0 && ha1 == hb1;
    const int lm = b->level_qmul[level];
    CoReq q;
    Operands o(q, who, be);
    o.in(ha0, level + 1, "a0"); o.in(ha1, level + 1, "a1"); o.in(hb0, level + 1, "b0"); o.in(hb1, level + 1, "b1");
    o.out(hout0, level + 1, "out0"); o.out(hout1, level + 1, "out1");
    o.out(k ? nullptr : o.poly(hout2), level + 1, "out2 (required when no relinearization key is given)");
    o.all_inplace = true;
    TRY(o.check());
    if (4L * o.B > 65535) return fail(HE_EINVAL, "%s: %d entries in one call, at most %d (split the batch)", who, o.B, 65535 / 4);
    ks_request(q, CO_BFV_MUL, ev, k, level, KS_FORM_COUNT, KsAlias{});
    q.obj = b.get(); q.par[1] = square;
    q.keep.push_back(b);
    q.run = [b, ev, k, level, lm, square](const View *v, int B) -> int {
        BasisExtender &be = *b->be;
        Ctx &ctx = *be.ctx;
        const int N = be.Q->N, nin = square ? 2 : 4;
        const size_t sQ = (size_t)(level + 1) * N, sM = (size_t)(lm + 1) * N, nB = (size_t)nin * B;
        const LimbTab tq = ident_tab(level + 1), tm = ident_tab(lm + 1, 0, 0, be.LQ);
        {
            Valu V(be.Q->logN);
            std::vector<int> dm;
            for (int j = 0; j <= lm; j++) dm.push_back(be.LQ + j);
            Valu I(be.Q->logN), P(be.Q->logN);  // per input component / per product
            for (int i = 0; i <= level; i++) I.ntt(cls_f64(be.small, i));
            valu_modup(I, be.small, 0, level + 1, dm);
            for (int j = 0; j <= lm; j++) I.ntt(cls_f64(be.small, be.LQ + j));
            for (int i = 0; i <= level; i++) { P.ntt(cls_f64(be.small, i), 2.0); P.mul(cls_f64(be.small, i), 2.0); }
            for (int j = 0; j <= lm; j++) { P.ntt(cls_f64(be.small, be.LQ + j)); P.mul(cls_f64(be.small, be.LQ + j), 2.0); }
            bfv_quantize_acct(*b, level, lm, P);
            for (int c = 0; c < 4; c++) V.v[c] = nin * I.v[c] + 3.0 * P.v[c];
            V.into(ctx, B);
        }
        const size_t extra = nB * (sQ + sM) + 3 * (size_t)B * (sQ + sM) + 3 * (size_t)B + 16;
        if (k) TRY(keyswitch_begin(*ev, *k, level, 6.0 * (level + 1), true, B, extra));  // 4 L in, 2 L out, the key
        else { ctx.acct(7.0 * (level + 1), 0, B, N); TRY(ctx.arena_reserve(extra)); }
        const View inQ{ctx.arena_take(nB * sQ), sQ}, inM{ctx.arena_take(nB * sM), sM};
        const View cQ{ctx.arena_take(3 * B * sQ), sQ}, cM{ctx.arena_take(3 * B * sM), sM};
        auto part = [B](const View &w, int c) { return View{w.p + (size_t)c * B * w.bstride, w.bstride}; };
        // modUpAndNTT (:991-1001): INTT of every component, ONE extension Q -> QMul and ONE lazy transform over all of them
        for (int c = 0; c < nin; c++) HIP_TRY(be_ntt(be, tq, v[c], part(inQ, c), B, true, NTT_REDUCE_INPUT));
        TRY(modup_between(be, true, level, lm, inQ, inM, 0, (int)nB));
        HIP_TRY(be_ntt(be, tm, inM, inM, (int)nB, false, NTT_LAZY_OUT | NTT_REDUCE_INPUT));
        // tensorLowDeg (:1003-1048) on Q and on QMul: MForm of the first operand, the three products; c1 is the canonical
        // representative of the reference's lazy sum (squaring: of its doubled product), which the inverse transform reduces anyway
        std::vector<uint64_t> r2(std::max(level, lm) + 1);
        for (int i = 0; i <= level; i++) r2[i] = be.Q->sub[i].mc.r2;
        HIP_TRY(launch_tensor(be.qp, tq, r2.data(), v[0], v[1], v[2], v[3], part(cQ, 0), part(cQ, 1), part(cQ, 2), B, ctx.stream));
        for (int j = 0; j <= lm; j++) r2[j] = be.P->sub[j].mc.r2;
        HIP_TRY(launch_tensor(be.qp, tm, r2.data(), part(inM, 0), part(inM, 1), part(inM, square ? 0 : 2), part(inM, square ? 1 : 3),
                              part(cM, 0), part(cM, 1), part(cM, 2), B, ctx.stream));
        // quantize (:1050-1071) of the three products at once
        HIP_TRY(be_ntt(be, tq, cQ, cQ, 3 * B, true, NTT_REDUCE_INPUT));
        HIP_TRY(be_ntt(be, tm, cM, cM, 3 * B, true, NTT_REDUCE_INPUT));
        TRY(bfv_quantize_launch(*b, level, cQ, cM, cQ, 3 * B));
        if (k) {
            // :966-969: the key switch of c2 with c0 / c1 as the ModDown epilogue's addends (the two ringQ.Add)
            HIP_TRY(be_ntt(be, tq, cQ, cQ, 3 * B, false, NTT_REDUCE_INPUT));
            const View c0 = part(cQ, 0), c1 = part(cQ, 1), c2 = part(cQ, 2);
            GpArgs g{&c2, nullptr, v[4], v[5], B, &c0, &c1, true};
            return key_switch(*ev, KS_GADGET_PRODUCT, level, *k, KsAlias{}, g);
        }
        // three outputs of the caller's: one transform whose stores go through an entry table (entry c B + e -> out_c, entry e)
        std::vector<size_t> off(3 * (size_t)B);
        for (int c = 0; c < 3; c++)
            for (int e = 0; e < B; e++) off[(size_t)c * B + e] = (size_t)(v[4 + c].p - v[4].p) + (size_t)e * v[4 + c].bstride;
        size_t *tab = reinterpret_cast<size_t *>(ctx.arena_take(off.size()));
        HIP_TRY(launch_tab_fill(tab, off.data(), (int)off.size(), ctx.stream));
        HIP_TRY(be_ntt(be, tq, cQ, View{v[4].p, 0, tab}, 3 * B, false, NTT_REDUCE_INPUT));
        return HE_OK;
    };
    q.one_by_one();  // (scratch-to-scratch launches: no entry tables)
    return co_dispatch(*be.ctx, o.B, q);
}

// ---------------------------------------------------------------------------------------
// CKKS encoder: Encode / Decode and the special FFT (include/hering_ckks_encoder.h; schemes/ckks/encoder.go, prec <= 53)
// ---------------------------------------------------------------------------------------
// Encoder (encoder.go:55-72) beside its rings: the table of roots and rotGroup on the device, the Garner constants of decode.
// The entries carry host data, so they run like he_poly_upload / he_poly_download: the calling thread's queued requests first
// (Scope), the launches straight on the context's stream, and the call returns when they are done.
struct CkksEncoder : Obj {
    std::shared_ptr<Ring> Q, P;
    int logM = 0, log_max_slots = 0;
    std::vector<double> roots;  // host copy, (M + 1) x 2
    double *d_roots = nullptr;
    uint32_t *d_rot = nullptr;
    uint64_t *d_garner = nullptr;  // g [cap][cap], then per level < cap: Q | Q >> 1 (2 cap words)
    int dec_levels = 0;            // levels he_ckks_decode serves: min(limbs of Q, cap)
    CkksEncoder() : Obj(T_CKKS_ENC) {}
    ~CkksEncoder() override {
        hipSetDevice(Q->ctx->dev);
        hipStreamSynchronize(Q->ctx->stream);
        if (d_roots) hipFree(d_roots);
        if (d_rot) hipFree(d_rot);
        if (d_garner) hipFree(d_garner);
    }
    CkksFftDev fft() const { return CkksFftDev{d_roots, d_rot, logM}; }
    const uint64_t *garner() const { return d_garner; }
    const uint64_t *qwords(int level) const { return d_garner + (size_t)kCkksDecodeMaxLimbs * kCkksDecodeMaxLimbs + (size_t)level * 2 * kCkksDecodeMaxLimbs; }
};
static bool all_finite(const double *v, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(v[i])) return false;
    return true;
}
int he_ckks_roots_host(uint64_t nth_root, double *out) {
    if (!out || nth_root < 8 || nth_root > (1ull << 22) || (nth_root & (nth_root - 1)))
        return fail(HE_EINVAL, "he_ckks_roots_host: NthRoot must be a power of two in [8, 2^22] and the output non-null");
    ckks_roots_complex128(nth_root, out);
    return HE_OK;
}
int he_ckks_encoder_create(he_handle hq, he_handle hp, const double *roots, he_handle *out) {
    static const char *who = "he_ckks_encoder_create";
    GET(Q, Ring, hq, T_RING);
    if (!out) return fail(HE_EINVAL, "%s: null output", who);
    auto e = std::make_shared<CkksEncoder>();
    e->Q = Q;
    if (hp) {
        e->P = get<Ring>(hp, T_RING);
        if (!e->P) return fail(HE_EHANDLE, "%s: bad ringP handle", who);
        if (e->P->ctx != Q->ctx || e->P->N != Q->N || e->P->type != Q->type)
            return fail(HE_EINVAL, "%s: ringP must share the context, degree and type of ringQ", who);
    }
    e->logM = Q->logN + (Q->type ? 2 : 1);
    e->log_max_slots = e->logM - 2;
    const size_t M = (size_t)1 << e->logM;
    e->roots.resize(2 * (M + 1));
    if (roots) {
        if (!all_finite(roots, 2 * (M + 1))) return fail(HE_EINVAL, "%s: the table of roots holds a non-finite word", who);
        memcpy(e->roots.data(), roots, 2 * (M + 1) * sizeof(double));
    } else {
        ckks_roots_complex128(M, e->roots.data());
    }
    const std::vector<uint32_t> rot = ckks_rot_group(M);
    e->dec_levels = std::min(Q->nmod(), kCkksDecodeMaxLimbs);
    std::vector<uint64_t> g = build_garner_table(Q->moduli, kCkksDecodeMaxLimbs);
    for (int l = 0; l < e->dec_levels; l++) {
        const std::vector<uint64_t> w = product_and_half_words(Q->moduli, l + 1, kCkksDecodeMaxLimbs);
        g.insert(g.end(), w.begin(), w.end());
    }
    Scope sc(Q->ctx.get());
    HIP_TRY(hipMalloc((void **)&e->d_roots, e->roots.size() * sizeof(double)));
    HIP_TRY(hipMemcpy(e->d_roots, e->roots.data(), e->roots.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc((void **)&e->d_rot, rot.size() * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(e->d_rot, rot.data(), rot.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc((void **)&e->d_garner, g.size() * sizeof(uint64_t)));
    HIP_TRY(hipMemcpy(e->d_garner, g.data(), g.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    *out = reg(e);
    return HE_OK;
}
int he_ckks_encoder_destroy(he_handle h) { return unreg(h, T_CKKS_ENC); }
int he_ckks_encoder_roots(he_handle h, double *out) {
    GET(e, CkksEncoder, h, T_CKKS_ENC);
    if (!out) return fail(HE_EINVAL, "he_ckks_encoder_roots: null output");
    memcpy(out, e->roots.data(), e->roots.size() * sizeof(double));
    return HE_OK;
}
int he_ckks_encoder_info(he_handle h, int out[4]) {
    GET(e, CkksEncoder, h, T_CKKS_ENC);
    if (!out) return fail(HE_EINVAL, "he_ckks_encoder_info: null output");
    out[0] = e->logM; out[1] = e->log_max_slots; out[2] = kCkksFftLdsLog; out[3] = kCkksDecodeMaxLimbs;
    return HE_OK;
}
// two device buffers of `words` doubles each from the scratch arena (the caller holds the context)
static int ckks_scratch(Ctx &c, size_t words, size_t extra, double **a, double **b, uint64_t **x) {
    TRY(c.arena_reserve((b ? 2 : 1) * words + extra + 8));
    *a = reinterpret_cast<double *>(c.arena_take(words));
    if (b) *b = reinterpret_cast<double *>(c.arena_take(words));
    if (x) *x = c.arena_take(extra);
    return HE_OK;
}
static int ckks_fft_api(he_handle h, int logn, int batch, double *values, bool inverse, const char *who) {
    GET(e, CkksEncoder, h, T_CKKS_ENC);
    if (logn < 0 || logn > e->log_max_slots) return fail(HE_EINVAL, "%s: logn (%d) must be in [0, %d]", who, logn, e->log_max_slots);
    if (!values || batch < 1 || batch > 65535) return fail(HE_EINVAL, "%s: null values or batch %d outside [1, 65535]", who, batch);
    const size_t words = ((size_t)batch << logn) * 2;
    if (!all_finite(values, words)) return fail(HE_EINVAL, "%s: non-finite input", who);
    Ctx &c = *e->Q->ctx;
    if (c.capturing) return fail(HE_EINVAL, "%s: host transfers cannot be captured in a graph", who);
    Scope sc(&c);
    double *a, *b;
    TRY(ckks_scratch(c, words, 0, &a, &b, nullptr));
    HIP_TRY(hipMemcpyAsync(a, values, words * 8, hipMemcpyHostToDevice, c.stream));
    HIP_TRY(launch_ckks_fft(e->fft(), a, b, a, logn, batch, inverse, nullptr, c.stream));
    HIP_TRY(hipMemcpyAsync(values, b, words * 8, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    return HE_OK;
}
int he_ckks_fft(he_handle enc, int logn, int batch, double *values) { return ckks_fft_api(enc, logn, batch, values, false, "he_ckks_fft"); }
int he_ckks_ifft(he_handle enc, int logn, int batch, double *values) { return ckks_fft_api(enc, logn, batch, values, true, "he_ckks_ifft"); }

// an output / input polynomial of an encoder entry: `limbs` limbs of the encoder's degree and context, `batch` entries (< 0: any)
static int ckks_poly(const CkksEncoder &e, he_handle h, int limbs, int batch, const char *name, const char *who, std::shared_ptr<Poly> *out) {
    auto p = get<Poly>(h, T_POLY);
    if (!p) return fail(HE_EHANDLE, "%s: bad polynomial handle for %s", who, name);
    if (p->ctx != e.Q->ctx) return fail(HE_EINVAL, "%s: %s belongs to another context", who, name);
    if (p->N != e.Q->N) return fail(HE_EINVAL, "%s: %s has degree %d, %d expected", who, name, p->N, e.Q->N);
    if (p->nlimbs < limbs) return fail(HE_EINVAL, "%s: %s has %d limbs, %d needed", who, name, p->nlimbs, limbs);
    if (batch >= 0 && p->batch != batch) return fail(HE_EINVAL, "%s: batch mismatch (%s has %d entries, %d expected)", who, name, p->batch, batch);
    if (p->batch > 65535) return fail(HE_EINVAL, "%s: %s has %d entries, at most 65535 per call", who, name, p->batch);
    *out = p;
    return HE_OK;
}
// Encode / Embed into outQ (and outP when level_p >= 0)
static int ckks_encode(const char *who, he_handle h, int level_q, int level_p, int log_slots, double scale, bool batched, bool is_ntt,
                       bool is_mont, const double *values, size_t n_values, bool cplx, int batch, he_handle hq, he_handle hp) {
    GET(e, CkksEncoder, h, T_CKKS_ENC);
    const Ring &Q = *e->Q;
    TRY(check_level(Q, level_q, who));
    if (level_p >= 0) {
        if (!e->P) return fail(HE_EINVAL, "%s: the encoder has no ringP", who);
        TRY(check_level(*e->P, level_p, who));
        if (hp == hq) return fail(HE_EINVAL, "%s: outP is outQ", who);
    }
    if (batch < 1 || batch > 65535) return fail(HE_EINVAL, "%s: batch %d outside [1, 65535]", who, batch);
    if (!values || n_values == 0) return fail(HE_EINVAL, "%s: no values", who);
    const size_t N = (size_t)Q.N;
    size_t slots = N;
    if (batched) {
        if (log_slots < 0 || log_slots > e->log_max_slots)  // encoder.go:221-223
            return fail(HE_EINVAL, "cannot Embed: logSlots (%d) must be greater or equal to %d and smaller than %d", log_slots, 0, e->log_max_slots);
        slots = (size_t)1 << log_slots;
        if (n_values > slots)  // :238-240
            return fail(HE_EINVAL, "cannot Embed: ensure that #values (%zu) <= slots (%zu) <= maxCols (%zu)", n_values, slots, (size_t)1 << e->log_max_slots);
    } else {
        if (cplx) return fail(HE_EINVAL, "cannot Encode: supported values.(type) for IsBatched=False is []float64");  // :179-181
        if (n_values > N) return fail(HE_EINVAL, "cannot Encode: maximum number of values is %zu but len(values) is %zu", N, n_values);  // :165-167
    }
    if (!std::isfinite(scale)) return fail(HE_EINVAL, "%s: the scale is not finite", who);
    if (!all_finite(values, (size_t)batch * n_values * (cplx ? 2 : 1))) return fail(HE_EINVAL, "%s: non-finite input", who);
    std::shared_ptr<Poly> oq, op;
    TRY(ckks_poly(*e, hq, level_q + 1, batch, "outQ", who, &oq));
    if (level_p >= 0) TRY(ckks_poly(*e, hp, level_p + 1, batch, "outP", who, &op));
    Ctx &c = *Q.ctx;
    if (c.capturing) return fail(HE_EINVAL, "%s: host transfers cannot be captured in a graph", who);

    // the vectors as the reference's buffer holds them before the transform: zero-padded (:309-312), the imaginary parts dropped
    // on a conjugate-invariant ring (:242-246); not batched: N reals
    const size_t per = batched ? 2 * slots : N, words = (size_t)batch * per;
    // (a full vector that needs neither padding nor its imaginary parts dropped goes to the device straight from the caller's buffer)
    const bool direct = n_values * (cplx ? 2 : 1) == per && (!batched || Q.type == 0);
    std::vector<double> host;
    if (!direct) {
        host.assign(words, 0.0);
        for (int b = 0; b < batch; b++) {
            const double *src = values + (size_t)b * n_values * (cplx ? 2 : 1);
            double *dst = host.data() + (size_t)b * per;
            if (!batched) memcpy(dst, src, n_values * sizeof(double));
            else if (cplx && Q.type == 0) memcpy(dst, src, 2 * n_values * sizeof(double));
            else for (size_t i = 0; i < n_values; i++) dst[2 * i] = src[cplx ? 2 * i : i];
        }
    }
    CkksQuantArgs qa;
    qa.mcQ = Q.dev.mc; qa.outQ = oq->view(); qa.nQ = level_q + 1;
    if (op) { qa.mcP = e->P->dev.mc; qa.outP = op->view(); qa.nP = level_p + 1; }
    qa.logN = Q.logN; qa.standard = Q.type == 0; qa.scale = scale;
    qa.log_gap = batched ? e->log_max_slots - log_slots : 0;

    const bool multipass = batched && log_slots > kCkksFftLdsLog;  // (only then do the values come back from the transform)
    Scope sc(&c);
    double *a, *b = nullptr;
    TRY(ckks_scratch(c, words, 0, &a, multipass ? &b : nullptr, nullptr));
    HIP_TRY(hipMemcpyAsync(a, direct ? values : host.data(), words * 8, hipMemcpyHostToDevice, c.stream));
    if (!batched) {
        HIP_TRY(launch_f64_to_rns(a, 0, true, qa, batch, c.stream));
    } else if (!multipass) {
        HIP_TRY(launch_ckks_fft(e->fft(), a, nullptr, nullptr, log_slots, batch, true, &qa, c.stream));  // IFFT + quantiser: one launch
    } else {
        HIP_TRY(launch_ckks_fft(e->fft(), a, b, a, log_slots, batch, true, nullptr, c.stream));
        HIP_TRY(launch_f64_to_rns(b, log_slots, false, qa, batch, c.stream));
    }
    // NTTSparseAndMontgomery (core/rlwe/utils.go:187-244): the transform of dimension n with the roots of N replicated gap times IS
    // the transform of the polynomial in Y = X^gap the quantiser wrote; the words are reduced on the way in, and the NTT of the
    // quirk words (q, an unreduced c) is the NTT of their residues.  MForm commutes with the transform (both outputs canonical).
    for (int side = 0; side < (op ? 2 : 1); side++) {
        const Ring &r = side ? *e->P : Q;
        const Poly &p = side ? *op : *oq;
        const int lv = side ? level_p : level_q;
        if (is_ntt) HIP_TRY(ring_ntt(r, ident_tab(lv + 1), p.view(), p.view(), batch, false, NTT_REDUCE_INPUT));
        if (batched && is_mont) HIP_TRY(launch_ew(r.dev, ident_tab(lv + 1), EW_MFORM, p.view(), p.view(), p.view(), batch, nullptr, nullptr, c.stream));
    }
    HIP_TRY(hipStreamSynchronize(c.stream));
    return HE_OK;
}
int he_ckks_encode(he_handle enc, int level, int log_slots, double scale, int is_batched, int is_ntt, int is_montgomery, const double *values,
                   size_t n_values, int is_complex, int batch, he_handle outQ) {
    return ckks_encode("he_ckks_encode", enc, level, -1, log_slots, scale, is_batched != 0, is_ntt != 0, is_montgomery != 0, values, n_values,
                       is_complex != 0, batch, outQ, 0);
}
int he_ckks_encode_qp(he_handle enc, int level_q, int level_p, int log_slots, double scale, int is_ntt, int is_montgomery, const double *values,
                      size_t n_values, int is_complex, int batch, he_handle outQ, he_handle outP) {
    return ckks_encode("he_ckks_encode_qp", enc, level_q, level_p < 0 ? -1 : level_p, log_slots, scale, true, is_ntt != 0, is_montgomery != 0, values,
                       n_values, is_complex != 0, batch, outQ, outP);
}
int he_ckks_decode(he_handle h, int level, int log_slots, double scale, int is_batched, int is_ntt, double logprec, he_handle hpt, int is_complex,
                   double *values) {
    static const char *who = "he_ckks_decode";
    GET(e, CkksEncoder, h, T_CKKS_ENC);
    const Ring &Q = *e->Q;
    TRY(check_level(Q, level, who));
    if (level + 1 > kCkksDecodeMaxLimbs) return fail(HE_EINVAL, "%s: %d limbs, at most %d are reconstructed", who, level + 1, kCkksDecodeMaxLimbs);
    if (is_batched && (log_slots < 0 || log_slots > e->log_max_slots))  // encoder.go:502-504
        return fail(HE_EINVAL, "cannot Decode: ensure that %d <= logSlots (%d) <= %d", 0, log_slots, e->log_max_slots);
    if (!values) return fail(HE_EINVAL, "%s: null output", who);
    if (!std::isfinite(scale) || scale == 0.0 || !std::isfinite(logprec)) return fail(HE_EINVAL, "%s: the scale must be finite and non-zero, logprec finite", who);
    std::shared_ptr<Poly> pt;
    TRY(ckks_poly(*e, hpt, level + 1, -1, "pt", who, &pt));
    Ctx &c = *Q.ctx;
    if (c.capturing) return fail(HE_EINVAL, "%s: host transfers cannot be captured in a graph", who);
    const int B = pt->batch;
    const size_t N = (size_t)Q.N, sQ = (size_t)(level + 1) * N;
    const size_t count = is_batched ? (size_t)1 << log_slots : N;
    const size_t words = (size_t)B * count * 2;

    CkksDecodeArgs da;
    da.nl = level + 1; da.log_slots = is_batched ? log_slots : 0; da.log_gap = is_batched ? e->log_max_slots - log_slots : 0;
    da.batched = is_batched != 0; da.standard = Q.type == 0; da.cplx = is_complex != 0; da.scale = scale;
    da.g = e->garner(); da.Qw = e->qwords(level);

    Scope sc(&c);
    double *a, *b;
    uint64_t *x = nullptr;
    TRY(ckks_scratch(c, words, is_ntt ? (size_t)B * sQ : 0, &a, &b, &x));
    View src = pt->view();
    if (is_ntt) {  // :508-512
        const View t{x, sQ};
        HIP_TRY(ring_ntt(Q, ident_tab(level + 1), src, t, B, true, NTT_REDUCE_INPUT));
        src = t;
    }
    HIP_TRY(launch_rns_to_f64(Q.dev, da, src, a, B, c.stream));
    if (!is_batched) {  // plaintextToFloat (:488-493, :757-759)
        HIP_TRY(hipMemcpyAsync(values, a, (size_t)B * N * (is_complex ? 2 : 1) * 8, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
        return HE_OK;
    }
    HIP_TRY(launch_ckks_fft(e->fft(), a, b, a, log_slots, B, false, nullptr, c.stream));
    std::vector<double> host(words);
    HIP_TRY(hipMemcpyAsync(host.data(), b, words * 8, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    if (logprec != 0) {  // :536-550: math.Round is half away from zero
        const double s = std::exp2(logprec);
        for (size_t i = 0; i < words; i++) host[i] = std::round(host[i] * s) / s;
    }
    if (is_complex) memcpy(values, host.data(), words * 8);
    else for (size_t i = 0; i < words / 2; i++) values[i] = host[2 * i];
    return HE_OK;
}

// ---------------------------------------------------------------------------------------
// BGV / BFV encoder: Encode / Decode, EncodeRingT / DecodeRingT, RingT2Q / RingQ2T (include/hering_bgv_encoder.h;
// schemes/bgv/encoder.go)
// ---------------------------------------------------------------------------------------
// Encoder (encoder.go:27-46) beside its rings.  On the device: the index matrix and its inverse, the Garner table with the words of
// Q and Q >> 1 per level, the constants of GenModUpConstants(Q[:level + 1], {T}) per level.  On the host: what the launches take as
// kernel arguments.  The entries run like he_poly_upload / he_poly_download: the calling thread's queued requests first (Scope),
// the launches straight on the context's stream, and the call returns when they are done.
struct BgvEncoder : Obj {
    std::shared_ptr<Ring> Q, P, T;
    int log_gap = 0;
    uint64_t t = 0;
    std::vector<uint64_t> perm;                // permuteMatrix(logN_T)
    uint32_t *d_perm = nullptr;                // [N_T] perm | [N_T] its inverse
    std::vector<uint64_t> tinvQ, tinvP;        // T^-1 mod q_i / p_j
    std::vector<uint64_t> tmodQ;               // MForm(T mod q_i)
    int q2t_levels = 0;                        // levels he_bgv_ring_q2t serves: min(limbs of Q, 32)
    uint64_t *d_garner = nullptr;              // as CkksEncoder::d_garner
    ConstPool pool;
    std::vector<ModUpRef> up;                  // [level], level >= 1
    std::vector<std::vector<uint64_t>> halfQ;  // [level][i]: (Q_level >> 1) mod q_i
    std::vector<uint64_t> halfT, qmodT;        // [level]: (Q_level >> 1) mod T, Q_level mod T
    std::vector<uint64_t> prodT;               // [i]: MForm_T(q_0 .. q_{i-1} mod T)
    BgvEncoder() : Obj(T_BGV_ENC) {}
    ~BgvEncoder() override {
        hipSetDevice(Q->ctx->dev);
        hipStreamSynchronize(Q->ctx->stream);
        if (d_perm) hipFree(d_perm);
        if (d_garner) hipFree(d_garner);
        pool.release();
    }
    int NT() const { return T->N; }
    const uint32_t *perm_dev() const { return d_perm; }
    const uint32_t *inv_dev() const { return d_perm + T->N; }
    const ModConst *mcT() const { return T->dev.mc; }
    uint64_t mont_t(uint64_t x) const { return to_mont(x % t, t); }
};
// permuteMatrix (encoder.go:110-133)
static std::vector<uint64_t> bgv_permute_matrix(int logN) {
    const uint64_t N = 1ull << logN, mask = 2 * N - 1;
    std::vector<uint64_t> perm(N);
    uint64_t pow = 1;
    for (uint64_t i = 0, j = N >> 1; i < (N >> 1); i++, j++) {
        uint64_t x = pow >> 1, pos = 0;  // BitReverse64(pow >> 1, logN)
        for (int b = 0; b < logN; b++, x >>= 1) pos = (pos << 1) | (x & 1);
        perm[i] = pos;
        perm[j] = N - pos - 1;
        pow = (pow * 5) & mask;
    }
    return perm;
}
int he_bgv_encoder_create(he_handle hq, he_handle hp, he_handle ht, he_handle *out) {
    static const char *who = "he_bgv_encoder_create";
    GET(Q, Ring, hq, T_RING);
    GET(T, Ring, ht, T_RING);
    if (!out) return fail(HE_EINVAL, "%s: null output", who);
    auto e = std::make_shared<BgvEncoder>();
    e->Q = Q; e->T = T;
    if (hp) {
        e->P = get<Ring>(hp, T_RING);
        if (!e->P) return fail(HE_EHANDLE, "%s: bad ringP handle", who);
        if (e->P->ctx != Q->ctx || e->P->N != Q->N || e->P->type != 0)
            return fail(HE_EINVAL, "%s: ringP must share the context and degree of ringQ and be of the standard type", who);
    }
    if (T->ctx != Q->ctx) return fail(HE_EINVAL, "%s: ringT belongs to another context", who);
    if (Q->type != 0 || T->type != 0) return fail(HE_EINVAL, "%s: the rings must be of the standard type", who);
    if (T->nmod() != 1) return fail(HE_EINVAL, "%s: ringT has %d moduli, exactly one expected", who, T->nmod());
    const uint64_t t = T->moduli[0];
    e->t = t;
    const int want = std::min(Q->logN, (int)__builtin_ctzll(t - 1) - 1);  // params.go:120-123
    if (T->logN != want) return fail(HE_EINVAL, "%s: ringT has logN %d, min(logN_Q, v2(T - 1) - 1) = %d expected", who, T->logN, want);
    for (const Ring *r : {Q.get(), e->P.get()})
        if (r)
            for (uint64_t q : r->moduli)
                if (std::gcd(q, t) != 1) return fail(HE_EINVAL, "%s: the plaintext modulus %llu is not coprime to the modulus %llu", who,
                                                     (unsigned long long)t, (unsigned long long)q);
    e->log_gap = Q->logN - T->logN;
    e->perm = bgv_permute_matrix(T->logN);
    const size_t NT = (size_t)T->N;
    std::vector<uint32_t> tab(2 * NT);
    for (size_t i = 0; i < NT; i++) { tab[i] = (uint32_t)e->perm[i]; tab[NT + e->perm[i]] = (uint32_t)i; }
    for (uint64_t q : Q->moduli) { e->tinvQ.push_back(invmod(t % q, q)); e->tmodQ.push_back(to_mont(t % q, q)); }
    if (e->P) for (uint64_t p : e->P->moduli) e->tinvP.push_back(invmod(t % p, p));
    e->q2t_levels = std::min(Q->nmod(), kBgvQ2TMaxLimbs);
    std::vector<uint64_t> g = build_garner_table(Q->moduli, kCkksDecodeMaxLimbs);
    e->up.resize(e->q2t_levels); e->halfQ.resize(e->q2t_levels); e->halfT.resize(e->q2t_levels); e->qmodT.resize(e->q2t_levels);
    uint64_t prod = 1;
    for (int l = 0; l < e->q2t_levels; l++) {
        const std::vector<uint64_t> S(Q->moduli.begin(), Q->moduli.begin() + l + 1);
        const std::vector<uint64_t> w = product_and_half_words(Q->moduli, l + 1, kCkksDecodeMaxLimbs);
        g.insert(g.end(), w.begin(), w.end());
        e->prodT.push_back(to_mont(prod, t));
        prod = mulmod(prod, Q->moduli[l] % t, t);
        e->qmodT[l] = prod;
        e->halfT[l] = half_product_mod(S, t);
        for (int i = 0; i <= l; i++) e->halfQ[l].push_back(half_product_mod(S, Q->moduli[i]));
        if (l >= 1) e->up[l] = pool_modup(e->pool, S, {t});  // encoder.go:62
    }
    Scope sc(Q->ctx.get());
    HIP_TRY(hipMalloc((void **)&e->d_perm, tab.size() * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(e->d_perm, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc((void **)&e->d_garner, g.size() * sizeof(uint64_t)));
    HIP_TRY(hipMemcpy(e->d_garner, g.data(), g.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    TRY(e->pool.upload());
    *out = reg(e);
    return HE_OK;
}
int he_bgv_encoder_destroy(he_handle h) { return unreg(h, T_BGV_ENC); }
int he_bgv_encoder_info(he_handle h, int out[4]) {
    GET(e, BgvEncoder, h, T_BGV_ENC);
    if (!out) return fail(HE_EINVAL, "he_bgv_encoder_info: null output");
    out[0] = e->T->logN; out[1] = e->log_gap; out[2] = kBgvQ2TMaxLimbs; out[3] = 0;
    return HE_OK;
}
int he_bgv_encoder_index(he_handle h, uint64_t *out) {
    GET(e, BgvEncoder, h, T_BGV_ENC);
    if (!out) return fail(HE_EINVAL, "he_bgv_encoder_index: null output");
    Scope sc(e->Q->ctx.get());
    std::vector<uint32_t> tab(e->NT());
    HIP_TRY(hipMemcpy(tab.data(), e->d_perm, tab.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < tab.size(); i++) out[i] = tab[i];
    return HE_OK;
}
// an operand of an encoder entry: a polynomial of `ring`'s degree and the encoder's context with `limbs` limbs, `batch` entries (< 0: any)
static int bgv_poly(const BgvEncoder &e, const Ring &ring, he_handle h, int limbs, int batch, const char *name, const char *who,
                    std::shared_ptr<Poly> *out) {
    auto p = get<Poly>(h, T_POLY);
    if (!p) return fail(HE_EHANDLE, "%s: bad polynomial handle for %s", who, name);
    if (p->ctx != e.Q->ctx) return fail(HE_EINVAL, "%s: %s belongs to another context", who, name);
    if (p->N != ring.N) return fail(HE_EINVAL, "%s: %s has degree %d, %d expected", who, name, p->N, ring.N);
    if (p->nlimbs < limbs) return fail(HE_EINVAL, "%s: %s has %d limbs, %d needed", who, name, p->nlimbs, limbs);
    if (batch >= 0 && p->batch != batch) return fail(HE_EINVAL, "%s: batch mismatch (%s has %d entries, %d expected)", who, name, p->batch, batch);
    if (p->batch > 65535) return fail(HE_EINVAL, "%s: %s has %d entries, at most 65535 per call", who, name, p->batch);
    *out = p;
    return HE_OK;
}
static int bgv_scale(const BgvEncoder &e, uint64_t scale, const char *who) {
    if (scale < 1 || scale >= e.t) return fail(HE_EINVAL, "%s: the scale (%llu) must be in [1, T)", who, (unsigned long long)scale);
    return HE_OK;
}
static int bgv_values(const BgvEncoder &e, const uint64_t *values, size_t n_values, int batch, const char *who) {
    if (batch < 1 || batch > 65535) return fail(HE_EINVAL, "%s: batch %d outside [1, 65535]", who, batch);
    if (!values || n_values == 0) return fail(HE_EINVAL, "%s: no values", who);
    if (n_values > (size_t)e.NT())  // encoder.go:163-165, :216-218
        return fail(HE_EINVAL, "%s: len(values)=%zu > slots=%d", who, n_values, e.NT());
    return HE_OK;
}
static int bgv_not_capturing(Ctx &c, const char *who) {
    if (c.capturing) return fail(HE_EINVAL, "%s: host transfers cannot be captured in a graph", who);
    return HE_OK;
}
// the launches of RingT2Q into limbs 0..level of oq (and 0..level_p of op): one fan-out; scale: the MulScalar of EncodeRingT folded in (0: none)
static int bgv_fanout(const BgvEncoder &e, View pT, uint64_t scale, bool scale_up, bool mont, const Ring *rq, const Poly *oq, int level_q,
                      const Ring *rp, const Poly *op, int level_p, bool q_is_p, int batch) {
    BgvFanoutArgs fa;
    auto constant = [&](uint64_t tinv, uint64_t q) {
        const uint64_t k = scale_up ? tinv : 1;
        return to_mont(mont ? to_mont(k, q) : k, q);
    };
    fa.mcQ = rq->dev.mc; fa.outQ = oq->view(); fa.nQ = level_q + 1;
    for (int i = 0; i <= level_q; i++) fa.cQ[i] = constant((q_is_p ? e.tinvP : e.tinvQ)[i], rq->moduli[i]);
    if (op) {
        fa.mcP = rp->dev.mc; fa.outP = op->view(); fa.nP = level_p + 1;
        for (int i = 0; i <= level_p; i++) fa.cP[i] = constant(e.tinvP[i], rp->moduli[i]);
    }
    fa.logN = e.Q->logN; fa.log_gap = e.log_gap;
    fa.scale_t = scale ? e.mont_t(scale) : 0;
    HIP_TRY(launch_bgv_t_to_rns(e.mcT(), pT, fa, batch, e.Q->ctx->stream));
    return HE_OK;
}
// values (host) -> dT (ring T, [batch][N_T]) on the stream: the upload and the scatter; inv: through the index matrix
static int bgv_scatter(const BgvEncoder &e, const uint64_t *values, size_t n_values, bool is_signed, bool through_index, uint64_t *d_vals, View dT,
                       int batch) {
    Ctx &c = *e.Q->ctx;
    HIP_TRY(hipMemcpyAsync(d_vals, values, (size_t)batch * n_values * 8, hipMemcpyHostToDevice, c.stream));
    HIP_TRY(launch_bgv_slots_to_t(e.mcT(), through_index ? e.inv_dev() : nullptr, d_vals, n_values, is_signed, dT, e.T->logN, batch, c.stream));
    return HE_OK;
}
int he_bgv_encode_ring_t(he_handle h, uint64_t scale, const uint64_t *values, size_t n_values, int is_signed, int batch, he_handle hpT) {
    static const char *who = "he_bgv_encode_ring_t";
    GET(e, BgvEncoder, h, T_BGV_ENC);
    TRY(bgv_scale(*e, scale, who));
    TRY(bgv_values(*e, values, n_values, batch, who));
    std::shared_ptr<Poly> pT;
    TRY(bgv_poly(*e, *e->T, hpT, 1, batch, "pT", who, &pT));
    Ctx &c = *e->Q->ctx;
    TRY(bgv_not_capturing(c, who));
    Scope sc(&c);
    TRY(c.arena_reserve((size_t)batch * n_values + 8));
    uint64_t *d_vals = c.arena_take((size_t)batch * n_values);
    TRY(bgv_scatter(*e, values, n_values, is_signed != 0, true, d_vals, pT->view(), batch));
    HIP_TRY(ring_ntt(*e->T, ident_tab(1), pT->view(), pT->view(), batch, true, 0));  // :258
    ScalarTab st;
    st.s[0] = e->mont_t(scale);
    HIP_TRY(launch_ew(e->T->dev, ident_tab(1), EW_MUL_SCALAR_MONT, pT->view(), pT->view(), pT->view(), batch, &st, nullptr, c.stream));  // :259
    HIP_TRY(hipStreamSynchronize(c.stream));
    return HE_OK;
}
// dT (ring T, scratch, [B][N_T]) -> values (host): [the NTT and the gather through the index matrix | the plain copy], centred when signed
static int bgv_gather(const BgvEncoder &e, View dT, bool through_index, bool is_signed, uint64_t *d_vals, uint64_t *values, int B) {
    Ctx &c = *e.Q->ctx;
    if (through_index) HIP_TRY(ring_ntt(*e.T, ident_tab(1), dT, dT, B, false, 0));  // :347
    HIP_TRY(launch_bgv_t_to_slots(e.mcT(), through_index ? e.perm_dev() : nullptr, dT, is_signed, d_vals, e.T->logN, B, c.stream));
    HIP_TRY(hipMemcpyAsync(values, d_vals, (size_t)B * e.NT() * 8, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    return HE_OK;
}
int he_bgv_decode_ring_t(he_handle h, uint64_t scale, he_handle hpT, int is_signed, uint64_t *values) {
    static const char *who = "he_bgv_decode_ring_t";
    GET(e, BgvEncoder, h, T_BGV_ENC);
    TRY(bgv_scale(*e, scale, who));
    if (!values) return fail(HE_EINVAL, "%s: null output", who);
    std::shared_ptr<Poly> pT;
    TRY(bgv_poly(*e, *e->T, hpT, 1, -1, "pT", who, &pT));
    Ctx &c = *e->Q->ctx;
    TRY(bgv_not_capturing(c, who));
    const int B = pT->batch;
    const size_t w = (size_t)B * e->NT();
    Scope sc(&c);
    TRY(c.arena_reserve(2 * w + 8));
    const View dT{c.arena_take(w), (size_t)e->NT()};
    uint64_t *d_vals = c.arena_take(w);
    ScalarTab st;
    st.s[0] = e->mont_t(invmod(scale, e->t));  // :346
    HIP_TRY(launch_ew(e->T->dev, ident_tab(1), EW_MUL_SCALAR_MONT, pT->view(), pT->view(), dT, B, &st, nullptr, c.stream));
    return bgv_gather(*e, dT, true, is_signed != 0, d_vals, values, B);
}
int he_bgv_ring_t2q(he_handle h, int level, int scale_up, int to_p, he_handle hpT, he_handle hout) {
    static const char *who = "he_bgv_ring_t2q";
    GET(e, BgvEncoder, h, T_BGV_ENC);
    if (to_p && !e->P) return fail(HE_EINVAL, "%s: the encoder has no ringP", who);
    const Ring &r = to_p ? *e->P : *e->Q;
    TRY(check_level(r, level, who));
    if (level + 1 > kMaxLimbs) return fail(HE_EINVAL, "%s: %d limbs, at most %d per call", who, level + 1, kMaxLimbs);
    std::shared_ptr<Poly> pT, po;
    TRY(bgv_poly(*e, *e->T, hpT, 1, -1, "pT", who, &pT));
    TRY(bgv_poly(*e, r, hout, level + 1, pT->batch, "pOut", who, &po));
    Ctx &c = *e->Q->ctx;
    TRY(bgv_not_capturing(c, who));
    Scope sc(&c);
    TRY(bgv_fanout(*e, pT->view(), 0, scale_up != 0, false, &r, po.get(), level, nullptr, nullptr, -1, to_p != 0, pT->batch));
    HIP_TRY(hipStreamSynchronize(c.stream));
    return HE_OK;
}
// RingQ2T of src (coefficient domain, limbs 0..level) into dT; post: MForm_T of the factor that follows (0: none)
static int bgv_q2t(const BgvEncoder &e, int level, bool scale_down, uint64_t post, View src, View dT, int B) {
    BgvQ2TArgs a;
    a.nl = level + 1; a.log_gap = e.log_gap; a.post = post;
    a.half_t = e.halfT[level]; a.q_mod_t = e.qmodT[level];
    a.g = e.d_garner;
    a.Qw = e.d_garner + (size_t)kCkksDecodeMaxLimbs * kCkksDecodeMaxLimbs + (size_t)level * 2 * kCkksDecodeMaxLimbs;
    for (int i = 0; i <= level; i++) {
        a.pre[i] = scale_down ? e.tmodQ[i] : 0;
        a.half_q[i] = e.halfQ[level][i];
        a.prod_t[i] = e.prodT[i];
    }
    for (int i = level + 1; i < kBgvQ2TMaxLimbs; i++) a.pre[i] = a.half_q[i] = a.prod_t[i] = 0;
    const ModUpDev up = level >= 1 ? e.up[level].on(e.pool) : ModUpDev{0, 0, nullptr, nullptr, nullptr};
    HIP_TRY(launch_bgv_rns_to_t(e.Q->dev, e.mcT(), up, a, src, dT, e.T->logN, B, e.Q->ctx->stream));
    return HE_OK;
}
static int bgv_q2t_level(const BgvEncoder &e, int level, const char *who) {
    TRY(check_level(*e.Q, level, who));
    if (level + 1 > kBgvQ2TMaxLimbs) return fail(HE_EINVAL, "%s: %d limbs, at most %d are reconstructed", who, level + 1, kBgvQ2TMaxLimbs);
    return HE_OK;
}
int he_bgv_ring_q2t(he_handle h, int level, int scale_down, he_handle hpQ, he_handle hpT) {
    static const char *who = "he_bgv_ring_q2t";
    GET(e, BgvEncoder, h, T_BGV_ENC);
    TRY(bgv_q2t_level(*e, level, who));
    std::shared_ptr<Poly> pQ, pT;
    TRY(bgv_poly(*e, *e->Q, hpQ, level + 1, -1, "pQ", who, &pQ));
    TRY(bgv_poly(*e, *e->T, hpT, 1, pQ->batch, "pT", who, &pT));
    Ctx &c = *e->Q->ctx;
    TRY(bgv_not_capturing(c, who));
    Scope sc(&c);
    TRY(bgv_q2t(*e, level, scale_down != 0, 0, pQ->view(), pT->view(), pQ->batch));
    HIP_TRY(hipStreamSynchronize(c.stream));
    return HE_OK;
}
// Encode / Embed into outQ (and outP when level_p >= 0)
static int bgv_encode(const char *who, he_handle h, int level_q, int level_p, uint64_t scale, bool batched, bool is_ntt, bool is_mont, bool scale_up,
                      const uint64_t *values, size_t n_values, bool is_signed, int batch, he_handle hq, he_handle hp) {
    GET(e, BgvEncoder, h, T_BGV_ENC);
    const Ring &Q = *e->Q;
    TRY(check_level(Q, level_q, who));
    if (level_q + 1 > kMaxLimbs) return fail(HE_EINVAL, "%s: %d limbs, at most %d per call", who, level_q + 1, kMaxLimbs);
    if (level_p >= 0) {
        if (!e->P) return fail(HE_EINVAL, "%s: the encoder has no ringP", who);
        TRY(check_level(*e->P, level_p, who));
        if (level_p + 1 > kMaxLimbs) return fail(HE_EINVAL, "%s: %d limbs, at most %d per call", who, level_p + 1, kMaxLimbs);
        if (hp == hq) return fail(HE_EINVAL, "%s: outP is outQ", who);
    }
    if (!batched && e->log_gap != 0)  // the reference handles only the first N_T of N words there (encoder.go:191)
        return fail(HE_EINVAL, "%s: the coefficient encoding needs N_T = N_Q (N_T = %d, N_Q = %d)", who, e->NT(), Q.N);
    TRY(bgv_scale(*e, scale, who));
    TRY(bgv_values(*e, values, n_values, batch, who));
    std::shared_ptr<Poly> oq, op;
    TRY(bgv_poly(*e, Q, hq, level_q + 1, batch, "outQ", who, &oq));
    if (level_p >= 0) TRY(bgv_poly(*e, *e->P, hp, level_p + 1, batch, "outP", who, &op));
    Ctx &c = *Q.ctx;
    TRY(bgv_not_capturing(c, who));
    const size_t wT = (size_t)batch * e->NT(), wV = (size_t)batch * n_values;
    Scope sc(&c);
    TRY(c.arena_reserve(wT + wV + 8));
    const View dT{c.arena_take(wT), (size_t)e->NT()};
    uint64_t *d_vals = c.arena_take(wV);
    TRY(bgv_scatter(*e, values, n_values, is_signed, batched, d_vals, dT, batch));
    if (batched) HIP_TRY(ring_ntt(*e->T, ident_tab(1), dT, dT, batch, true, 0));  // :258
    // :259 / :191 (MulScalar modulo T), RingT2Q and, batched, MForm (:292, :308, :325) in one launch; not batched: no MForm
    TRY(bgv_fanout(*e, dT, scale, scale_up, batched && is_mont, &Q, oq.get(), level_q, e->P.get(), op.get(), level_p, false, batch));
    if (is_ntt) {
        HIP_TRY(ring_ntt(Q, ident_tab(level_q + 1), oq->view(), oq->view(), batch, false, 0));
        if (op) HIP_TRY(ring_ntt(*e->P, ident_tab(level_p + 1), op->view(), op->view(), batch, false, 0));
    }
    HIP_TRY(hipStreamSynchronize(c.stream));
    return HE_OK;
}
int he_bgv_encode(he_handle enc, int level, uint64_t scale, int is_batched, int is_ntt, int is_montgomery, int scale_up, const uint64_t *values,
                  size_t n_values, int is_signed, int batch, he_handle outQ) {
    return bgv_encode("he_bgv_encode", enc, level, -1, scale, is_batched != 0, is_ntt != 0, is_montgomery != 0, scale_up != 0, values, n_values,
                      is_signed != 0, batch, outQ, 0);
}
int he_bgv_encode_qp(he_handle enc, int level_q, int level_p, uint64_t scale, int is_ntt, int is_montgomery, int scale_up, const uint64_t *values,
                     size_t n_values, int is_signed, int batch, he_handle outQ, he_handle outP) {
    return bgv_encode("he_bgv_encode_qp", enc, level_q, level_p < 0 ? -1 : level_p, scale, true, is_ntt != 0, is_montgomery != 0, scale_up != 0, values,
                      n_values, is_signed != 0, batch, outQ, outP);
}
int he_bgv_decode(he_handle h, int level, uint64_t scale, int is_batched, int is_ntt, he_handle hpt, int is_signed, uint64_t *values) {
    static const char *who = "he_bgv_decode";
    GET(e, BgvEncoder, h, T_BGV_ENC);
    const Ring &Q = *e->Q;
    TRY(bgv_q2t_level(*e, level, who));
    if (!is_batched && e->log_gap != 0)  // encoder.go:496-518
        return fail(HE_EINVAL, "%s: the coefficient encoding needs N_T = N_Q (N_T = %d, N_Q = %d)", who, e->NT(), Q.N);
    TRY(bgv_scale(*e, scale, who));
    if (!values) return fail(HE_EINVAL, "%s: null output", who);
    std::shared_ptr<Poly> pt;
    TRY(bgv_poly(*e, Q, hpt, level + 1, -1, "pt", who, &pt));
    Ctx &c = *Q.ctx;
    TRY(bgv_not_capturing(c, who));
    const int B = pt->batch;
    const size_t sQ = (size_t)(level + 1) * Q.N, wT = (size_t)B * e->NT();
    Scope sc(&c);
    TRY(c.arena_reserve(2 * wT + (is_ntt ? (size_t)B * sQ : 0) + 8));
    const View dT{c.arena_take(wT), (size_t)e->NT()};
    uint64_t *d_vals = c.arena_take(wT);
    View src = pt->view();
    if (is_ntt) {  // :481-487
        const View x{c.arena_take((size_t)B * sQ), sQ};
        HIP_TRY(ring_ntt(Q, ident_tab(level + 1), src, x, B, true, NTT_REDUCE_INPUT));
        src = x;
    }
    TRY(bgv_q2t(*e, level, true, e->mont_t(invmod(scale, e->t)), src, dT, B));  // RingQ2T, then the MulScalar of :346 / :496
    return bgv_gather(*e, dT, is_batched != 0, is_signed != 0, d_vals, values, B);
}

// ---------------------------------------------------------------------------------------
// the randomness source and the ring samplers (include/hering_sampler.h; ring/sampler_uniform.go, sampler_gaussian.go,
// sampler_ternary.go)
// ---------------------------------------------------------------------------------------
// sampling.PRNG: `buf` holds the bytes fetched and not yet consumed, `pos` the bytes consumed in the reference's sense.  One call
// at a time per handle (mu): the order of the Reads on a source is the caller's to fix, as with the reference's samplers.
struct Prng : Obj {
    he_prng_read_fn read = nullptr;  // null: getrandom(2)
    void *user = nullptr;
    std::vector<uint8_t> buf;
    uint64_t pos = 0;
    std::mutex mu;
    Prng() : Obj(T_PRNG) {}
    ~Prng() override { wipe_all(); }
    // the whole block: erase() and resize() leave earlier copies of fetched bytes beyond size()
    void wipe_all() {
        const size_t n = buf.size();
        buf.resize(buf.capacity());
        wipe(buf.data(), buf.size());
        buf.resize(n);
    }
    static void wipe(void *p, size_t n) {
        if (n) explicit_bzero(p, n);
    }
    // have at least `want` bytes in buf
    int fetch(size_t want, const char *who) {
        const size_t have = buf.size();
        if (want <= have) return HE_OK;
        if (buf.capacity() < want) {  // grow by hand: the old block is wiped before it is released
            std::vector<uint8_t> next;
            next.reserve(want + want / 2);
            next.assign(buf.begin(), buf.end());
            wipe_all();
            buf.swap(next);
        }
        buf.resize(want);
        uint8_t *dst = buf.data() + have;
        size_t n = want - have;
        if (read) {
            if (read(user, dst, n) != 0) {
                buf.resize(have);
                return fail(HE_EPRNG, "%s: the source's reader failed or ran short of %zu bytes", who, n);
            }
            return HE_OK;
        }
        while (n) {
            const ssize_t got = getrandom(dst, std::min(n, (size_t)1 << 24), 0);
            if (got < 0 && errno == EINTR) continue;
            if (got <= 0) {
                buf.resize(have);
                return fail(HE_EPRNG, "%s: getrandom failed (%s)", who, strerror(errno));
            }
            dst += got;
            n -= (size_t)got;
        }
        return HE_OK;
    }
    void consume(size_t n) {
        const size_t old = buf.size();
        buf.erase(buf.begin(), buf.begin() + n);  // (the tail moves down: its old copy stays in [size, old))
        buf.resize(old);
        wipe(buf.data() + old - n, n);
        buf.resize(old - n);
        pos += n;
    }
};
int he_prng_create_system(he_handle *out) {
    if (!out) return fail(HE_EINVAL, "he_prng_create_system: null output");
    *out = reg(std::make_shared<Prng>());
    return HE_OK;
}
int he_prng_create_callback(he_prng_read_fn read, void *user, he_handle *out) {
    if (!out || !read) return fail(HE_EINVAL, "he_prng_create_callback: null %s", out ? "reader" : "output");
    auto g = std::make_shared<Prng>();
    g->read = read;
    g->user = user;
    *out = reg(g);
    return HE_OK;
}
int he_prng_destroy(he_handle h) { return unreg(h, T_PRNG); }
int he_prng_position(he_handle h, uint64_t out[2]) {
    GET(g, Prng, h, T_PRNG);
    if (!out) return fail(HE_EINVAL, "he_prng_position: null output");
    std::lock_guard<std::mutex> lk(g->mu);
    out[0] = g->pos;
    out[1] = g->buf.size();
    return HE_OK;
}
int he_gaussian_tables_host(uint32_t out[384]) {
    if (!out) return fail(HE_EINVAL, "he_gaussian_tables_host: null output");
    gaussian_ziggurat_tables(out);
    return HE_OK;
}
static int ternary_density(double p, const char *who) {
    if (!(p > 0.0 && p < 1.0)) return fail(HE_EINVAL, "%s: the density P = %g is not in (0, 1)", who, p);
    return HE_OK;
}
int he_ternary_matrix_host(double p, uint64_t out[2]) {
    TRY(ternary_density(p, "he_ternary_matrix_host"));
    if (!out) return fail(HE_EINVAL, "he_ternary_matrix_host: null output");
    ternary_matrix_words(1 - p, out[0], out[1]);
    return HE_OK;
}
// an output of a sampler entry: limbs 0..level of a polynomial of `r`
static int sampler_poly(const Ring &r, int level, he_handle h, int batch, const char *name, const char *who, std::shared_ptr<Poly> *out) {
    TRY(check_level(r, level, who));
    if (level + 1 > kMaxLimbs) return fail(HE_EINVAL, "%s: %d limbs, at most %d per call", who, level + 1, kMaxLimbs);
    auto p = get<Poly>(h, T_POLY);
    if (!p) return fail(HE_EHANDLE, "%s: bad polynomial handle for %s", who, name);
    if (p->ctx != r.ctx) return fail(HE_EINVAL, "%s: %s belongs to another context", who, name);
    if (p->N != r.N) return fail(HE_EINVAL, "%s: %s has degree %d, %d expected", who, name, p->N, r.N);
    if (p->nlimbs < level + 1) return fail(HE_EINVAL, "%s: %s has %d limbs, %d needed", who, name, p->nlimbs, level + 1);
    if (batch >= 0 && p->batch != batch) return fail(HE_EINVAL, "%s: batch mismatch (%s has %d entries, %d expected)", who, name, p->batch, batch);
    if (p->batch > 65535) return fail(HE_EINVAL, "%s: %s has %d entries, at most 65535 per call", who, name, p->batch);
    *out = p;
    return HE_OK;
}
// One sampler call: fetch, stage, parse, and again with twice the stream while the parse runs out of it.  `first` bytes are
// fetched before the first attempt, and the call gives up once an attempt would need more than 64 `expected`.  parse(stream, bytes,
// status) enqueues the launches that read the stream and write status (kernels.h); it writes only scratch or words that a later
// attempt rewrites, so an attempt can be abandoned.  finish() enqueues what follows a parse that succeeded.  Every scratch region
// that held stream bytes or sampled values is zeroed on the stream before the call returns.
struct SamplerScratch {
    size_t words = 0;           // beside the stream and the status words
    uint64_t *p = nullptr;
};
static int sampler_run(const char *who, Ctx &c, Prng &g, size_t expected, size_t first, SamplerScratch &scratch,
                       const std::function<int(const uint64_t *, size_t, uint64_t *, uint64_t *)> &parse, const std::function<int()> &finish) {
    if (c.capturing) return fail(HE_EINVAL, "%s: host transfers cannot be captured in a graph", who);
    std::lock_guard<std::mutex> lk(g.mu);
    Scope sc(&c);
    const size_t cap = expected * 64;
    uint64_t st[4] = {0, 0, 0, 0};
    int rc = HE_OK;
    size_t staged = 0;
    uint64_t *d_stream = nullptr;
    for (size_t want = first;; want *= 2) {
        if (want > cap) {
            rc = fail(HE_EPRNG, "%s: the source did not let the call finish within %zu bytes (64 times the expected %zu)", who, cap, expected);
            break;
        }
        if ((rc = g.fetch(want, who)) != HE_OK) break;
        const size_t sw = (want + 7) / 8;
        c.arena_reset();
        if (staged) HIP_TRY(hipMemsetAsync(d_stream, 0, staged * 8, c.stream));  // (the arena may move below)
        if ((rc = c.arena_reserve(sw + 4 + scratch.words + 8)) != HE_OK) break;
        d_stream = c.arena_take(sw);
        uint64_t *d_status = c.arena_take(4);
        scratch.p = c.arena_take(scratch.words);
        staged = sw;
        HIP_TRY(hipMemsetAsync(d_stream + sw - 1, 0, 8, c.stream));
        HIP_TRY(hipMemcpyAsync(d_stream, g.buf.data(), want, hipMemcpyHostToDevice, c.stream));
        HIP_TRY(hipMemsetAsync(d_status, 0, 32, c.stream));
        if ((rc = parse(d_stream, want, d_status, st)) != HE_OK) break;
        if (st[0] == 0) break;
        if (st[0] == 2) {
            rc = fail(HE_EINVAL, "%s: a Knuth-Yao walk reached column 55 of the probability matrix (an index panic in the reference)", who);
            break;
        }
    }
    if (rc == HE_OK) rc = finish();
    if (d_stream) {
        (void)hipMemsetAsync(d_stream, 0, staged * 8, c.stream);
        if (scratch.words) (void)hipMemsetAsync(scratch.p, 0, scratch.words * 8, c.stream);
    }
    HIP_TRY(hipStreamSynchronize(c.stream));
    if (rc != HE_OK) return rc;
    if (st[1] > g.buf.size()) return fail(HE_EDEVICE, "%s: the parse consumed %llu bytes of %zu", who, (unsigned long long)st[1], g.buf.size());
    g.consume((size_t)st[1]);
    return HE_OK;
}
// the status words of the attempt, on the host
static int sampler_status(Ctx &c, const uint64_t *d_status, uint64_t *st) {
    HIP_TRY(hipMemcpyAsync(st, d_status, 32, hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    return HE_OK;
}
static int uniform_read_run(const char *who, Ctx &c, Prng &g, int N, int B, int nparts, const ModConst *const mc[2], const int nl[2],
                            uint64_t *const out[2], const size_t bs[2], bool add, const std::function<int(uint64_t *)> &sum);
int he_sampler_uniform_read(he_handle hr, int level, he_handle hrp, int levelP, he_handle hg, int add, he_handle hpol, he_handle hpolP) {
    static const char *who = "he_sampler_uniform_read";
    GET(r, Ring, hr, T_RING);
    GET(g, Prng, hg, T_PRNG);
    std::shared_ptr<Ring> rp;
    std::shared_ptr<Poly> pol, polP;
    TRY(sampler_poly(*r, level, hpol, -1, "pol", who, &pol));
    if (hrp) {
        rp = get<Ring>(hrp, T_RING);
        if (!rp) return fail(HE_EHANDLE, "%s: bad ringP handle", who);
        if (rp->ctx != r->ctx || rp->N != r->N) return fail(HE_EINVAL, "%s: ringP must share the context and degree of the ring", who);
        TRY(sampler_poly(*rp, levelP, hpolP, pol->batch, "polP", who, &polP));
        if (polP == pol) return fail(HE_EINVAL, "%s: pol and polP are one polynomial", who);
    }
    Ctx &c = *r->ctx;
    const int N = r->N, B = pol->batch, nparts = rp ? 2 : 1;
    const int nl[2] = {level + 1, rp ? levelP + 1 : 0};
    const size_t words[2] = {(size_t)nl[0] * N, (size_t)nl[1] * N};
    const ModConst *const mc[2] = {r->dev.mc, rp ? rp->dev.mc : nullptr};
    uint64_t *const out[2] = {pol->d, rp ? polP->d : nullptr};
    const size_t bs[2] = {pol->view().bstride, rp ? polP->view().bstride : 0};
    auto sum = [&](uint64_t *drawn) -> int {  // ReadAndAdd: the sum is a launch of its own, per part
        const View t0{drawn, words[0]};
        HIP_TRY(launch_ew(r->dev, ident_tab(nl[0]), EW_ADD, pol->view(), t0, pol->view(), B, nullptr, nullptr, c.stream));
        if (rp) {
            const View t1{drawn + (size_t)B * words[0], words[1]};
            HIP_TRY(launch_ew(rp->dev, ident_tab(nl[1]), EW_ADD, polP->view(), t1, polP->view(), B, nullptr, nullptr, c.stream));
        }
        return HE_OK;
    };
    return uniform_read_run(who, c, *g, N, B, nparts, mc, nl, out, bs, add != 0, sum);
}
// The Reads of one uniform call into raw storage: part k (k < nparts) into limbs 0..nl[k]-1 of the B entries at out[k], bs[k] words
// apart, with the modulus records mc[k].  add: the draw lands in scratch (part 0's B entries, then part 1's) and sum(scratch) adds it.
static int uniform_read_run(const char *who, Ctx &c, Prng &g, int N, int B, int nparts, const ModConst *const mc[2], const int nl[2],
                            uint64_t *const out[2], const size_t bs[2], bool add, const std::function<int(uint64_t *)> &sum) {
    const size_t words[2] = {(size_t)nl[0] * N, nparts > 1 ? (size_t)nl[1] * N : 0};
    const size_t entry_bytes = 8 * ((((words[0] + 127) & ~(size_t)127)) + ((words[1] + 127) & ~(size_t)127));
    SamplerScratch scratch;
    if (add) scratch.words = (size_t)B * (words[0] + words[1]);  // ReadAndAdd: the draw lands here and is added when the parse is through
    SamplerPart parts[2];
    auto set_parts = [&]() {
        parts[0] = SamplerPart{mc[0], add ? scratch.p : out[0], add ? words[0] : bs[0], nl[0]};
        if (nparts > 1) parts[1] = SamplerPart{mc[1], add ? scratch.p + (size_t)B * words[0] : out[1], add ? words[1] : bs[1], nl[1]};
    };
    bool direct = true;  // the one-thread-per-word launch, until a word is rejected
    auto parse = [&](const uint64_t *d_stream, size_t bytes, uint64_t *d_status, uint64_t *st) -> int {
        set_parts();
        if (direct) {
            HIP_TRY(launch_sampler_uniform(d_stream, bytes / 8, parts, nparts, N, B, false, d_status, c.stream));
            TRY(sampler_status(c, d_status, st));
            if (st[2] == 0) {
                st[1] = (uint64_t)B * entry_bytes;
                return HE_OK;
            }
            direct = false;
        }
        HIP_TRY(launch_sampler_uniform(d_stream, bytes / 8, parts, nparts, N, B, true, d_status, c.stream));
        return sampler_status(c, d_status, st);
    };
    auto finish = [&]() -> int { return add ? sum(scratch.p) : HE_OK; };
    return sampler_run(who, c, g, (size_t)B * entry_bytes, (size_t)B * entry_bytes, scratch, parse, finish);
}
// The parse of one Gaussian call: the small values of B entries (launch_sampler_gaussian's words) in scratch, handed to finish(vals),
// which enqueues what becomes of them; they are zeroed before the call returns.
static int gaussian_parse_run(const char *who, Ctx &c, Prng &g, int N, int B, double sigma, double bound, const std::function<int(const uint64_t *)> &use);
// the launches after the parse of a Gaussian or ternary call: the small values into limbs 0..level of pol
int he_sampler_gaussian_read(he_handle hr, int level, he_handle hg, double sigma, double bound, int montgomery, int add, he_handle hpol) {
    static const char *who = "he_sampler_gaussian_read";
    GET(r, Ring, hr, T_RING);
    GET(g, Prng, hg, T_PRNG);
    std::shared_ptr<Poly> pol;
    TRY(sampler_poly(*r, level, hpol, -1, "pol", who, &pol));
    if (!(sigma > 0.0) || sigma > 0x1p53)  // sampler_gaussian.go:100: beyond, the reference leaves float64 when the bound is large too
        return fail(HE_EINVAL, "%s: sigma = %g is not in (0, 2^53] (the arbitrary-precision branch is not built)", who, sigma);
    if (!(bound >= 0.0) || bound > 0x1p62) return fail(HE_EINVAL, "%s: bound = %g is not in [0, 2^62]", who, bound);
    Ctx &c = *r->ctx;
    const int N = r->N, B = pol->batch;
    return gaussian_parse_run(who, c, *g, N, B, sigma, bound, [&](const uint64_t *vals) -> int {
        HIP_TRY(launch_sampler_expand(r->dev.mc, vals, true, add != 0, montgomery != 0, nullptr, nullptr, pol->view(), N, level + 1, B, c.stream));
        return HE_OK;
    });
}
static int gaussian_parse_run(const char *who, Ctx &c, Prng &g, int N, int B, double sigma, double bound, const std::function<int(const uint64_t *)> &use) {
    const size_t entry = ((size_t)N * 8 + 1023) & ~(size_t)1023, ahead = ((size_t)N * 8 + N / 2 + 2047) & ~(size_t)1023;
    SamplerScratch scratch;
    scratch.words = (size_t)B * N + 192;
    auto parse = [&](const uint64_t *d_stream, size_t bytes, uint64_t *d_status, uint64_t *st) -> int {
        static const std::array<uint32_t, 384> tab = [] { std::array<uint32_t, 384> t; gaussian_ziggurat_tables(t.data()); return t; }();
        uint32_t *d_tab = reinterpret_cast<uint32_t *>(scratch.p + (size_t)B * N);
        HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), sizeof tab, hipMemcpyHostToDevice, c.stream));
        HIP_TRY(launch_sampler_gaussian(d_stream, bytes / 8, d_tab, sigma, bound, scratch.p, N, B, d_status, c.stream));
        return sampler_status(c, d_status, st);
    };
    auto finish = [&]() -> int { return use(scratch.p); };
    return sampler_run(who, c, g, (size_t)B * entry, (size_t)B * ahead, scratch, parse, finish);
}
// sampleProba: the two-bit form (half) or the Knuth-Yao walk over the rows cut from x0 / x1
static int ternary_run(const char *who, he_handle hr, int level, he_handle hg, bool half, uint64_t x0, uint64_t x1, int montgomery, int add,
                       he_handle hpol) {
    GET(r, Ring, hr, T_RING);
    GET(g, Prng, hg, T_PRNG);
    std::shared_ptr<Poly> pol;
    TRY(sampler_poly(*r, level, hpol, -1, "pol", who, &pol));
    Ctx &c = *r->ctx;
    const int N = r->N, B = pol->batch;
    uint64_t lut1[kMaxLimbs], lut2[kMaxLimbs];  // matrixValues[i][1], [2] (:82-104)
    for (int i = 0; i <= level; i++) {
        const uint64_t q = r->moduli[i];
        lut1[i] = montgomery ? to_mont(1, q) : 1;
        lut2[i] = montgomery ? to_mont(q - 1, q) : q - 1;
    }
    const size_t entry = half ? (size_t)N / 4 : (size_t)N;
    SamplerScratch scratch;
    scratch.words = (size_t)B * N;
    auto parse = [&](const uint64_t *d_stream, size_t bytes, uint64_t *d_status, uint64_t *st) -> int {
        HIP_TRY(launch_sampler_ternary(reinterpret_cast<const uint8_t *>(d_stream), bytes, half, x0, x1, scratch.p, N, B, d_status, c.stream));
        if (half) {
            st[0] = 0;
            st[1] = (uint64_t)B * entry;
            return HE_OK;
        }
        return sampler_status(c, d_status, st);
    };
    auto finish = [&]() -> int {
        HIP_TRY(launch_sampler_expand(r->dev.mc, scratch.p, false, add != 0, false, lut1, lut2, pol->view(), N, level + 1, B, c.stream));
        return HE_OK;
    };
    return sampler_run(who, c, *g, (size_t)B * entry, (size_t)B * entry, scratch, parse, finish);
}
int he_sampler_ternary_read(he_handle hr, int level, he_handle hg, double p, int montgomery, int add, he_handle hpol) {
    static const char *who = "he_sampler_ternary_read";
    TRY(ternary_density(p, who));
    const double inv_density = 1 - p;  // sampler_ternary.go:34
    uint64_t x0 = 0, x1 = 0;
    if (inv_density != 0.5) ternary_matrix_words(inv_density, x0, x1);
    return ternary_run(who, hr, level, hg, inv_density == 0.5, x0, x1, montgomery, add, hpol);
}
int he_debug_sampler_ternary_words(he_handle hr, int level, he_handle hg, uint64_t x0, uint64_t x1, int montgomery, int add, he_handle hpol) {
    return ternary_run("he_debug_sampler_ternary_words", hr, level, hg, false, x0, x1, montgomery, add, hpol);
}

// ---------------------------------------------------------------------------------------
// rlwe.Encryptor and rlwe.Decryptor (include/hering_encryptor.h; core/rlwe/encryptor.go, decryptor.go): compositions of the public
// entries above, nothing fused.  Each object registers handles of its own for the evaluator, its rings and its basis extender, so
// that the caller's may be destroyed first.
// ---------------------------------------------------------------------------------------
struct RlweFrame {
    std::shared_ptr<Evaluator> ev;
    he_handle hev = 0, hq = 0, hp = 0, hbe = 0;  // hp = 0: no special primes
    void bind(const std::shared_ptr<Evaluator> &e) {
        ev = e;
        hev = reg(e);
        hbe = reg(e->be);
        hq = reg(e->be->Q);
        if (!e->be->P->moduli.empty()) hp = reg(e->be->P);
    }
    ~RlweFrame() {
        for (he_handle h : {hev, hq, hp, hbe})
            if (h) reg_drop(h);
    }
    Ctx &ctx() const { return *ev->be->ctx; }
    int maxP() const { return (int)ev->be->P->moduli.size() - 1; }
    int maxQ() const { return (int)ev->be->Q->moduli.size() - 1; }
};
struct Encryptor : Obj, RlweFrame {
    std::shared_ptr<Prng> prng_keep;
    he_handle prng = 0;
    double xs_p = 0, sigma = 0, bound = 0;
    std::mutex mu;  // the key binding
    int kind = 0;
    he_handle key[4] = {0, 0, 0, 0};
    Encryptor() : Obj(T_ENCRYPTOR) {}
    ~Encryptor() override {
        if (prng) reg_drop(prng);
    }
};
struct Decryptor : Obj, RlweFrame {
    he_handle sk = 0;
    Decryptor() : Obj(T_DECRYPTOR) {}
};
// a temporary of a composed entry: cleared before it goes back to the pool (it held u, e or a masked plaintext)
struct TmpPoly {
    he_handle h = 0;
    int alloc(he_handle ring, int limbs, int batch) { return he_poly_alloc_scratch(ring, limbs, batch, &h); }
    ~TmpPoly() {
        if (h) {
            (void)he_poly_zero(h);
            (void)he_poly_free(h);
        }
    }
};
// every output distinct from every other output and from every other operand (0: an absent operand)
static int rlwe_distinct(const char *who, const he_handle *outs, int nouts, const he_handle *others, int nothers) {
    auto mem = [](he_handle h) -> const void * {
        auto p = h ? get<Poly>(h, T_POLY) : nullptr;
        return p ? (const void *)p->d : nullptr;
    };
    for (int i = 0; i < nouts; i++) {
        const void *a = mem(outs[i]);
        if (!a) continue;
        for (int j = i + 1; j < nouts; j++)
            if (mem(outs[j]) == a) return fail(HE_EINVAL, "%s: outputs %d and %d are one polynomial", who, i, j);
        for (int j = 0; j < nothers; j++)
            if (mem(others[j]) == a) return fail(HE_EINVAL, "%s: output %d is also an input or a key polynomial (operand %d)", who, i, j);
    }
    return HE_OK;
}
static int rlwe_frame_begin(Ctx &c, const char *who) {
    if (c.capturing) return fail(HE_EINVAL, "%s: host transfers cannot be captured in a graph", who);
    return HE_OK;
}
static int rlwe_frame_end(Ctx &c) {  // the call returns with its device work finished
    Scope sc(&c);
    HIP_TRY(hipStreamSynchronize(c.stream));
    return HE_OK;
}
static int batch_of(he_handle h, const char *who, int *B) {
    auto p = get<Poly>(h, T_POLY);
    if (!p) return fail(HE_EHANDLE, "%s: bad Poly handle %llu", who, (unsigned long long)h);
    *B = p->batch;
    return HE_OK;
}

int he_encryptor_create(he_handle hev, he_handle hprng, double xs_p, double xe_sigma, double xe_bound, he_handle *out) {
    static const char *who = "he_encryptor_create";
    GET(ev, Evaluator, hev, T_EVAL);
    GET(g, Prng, hprng, T_PRNG);
    if (!out) return fail(HE_EINVAL, "%s: null output", who);
    TRY(ternary_density(xs_p, who));
    if (!(xe_sigma > 0.0) || xe_sigma > 0x1p53 || !(xe_bound >= 0.0) || xe_bound > 0x1p62)
        return fail(HE_EINVAL, "%s: Xe = {%g, %g}: sigma in (0, 2^53] and bound in [0, 2^62] (hering_sampler.h)", who, xe_sigma, xe_bound);
    auto e = std::make_shared<Encryptor>();
    e->bind(ev);
    e->prng_keep = g;
    e->prng = reg(g);
    e->xs_p = xs_p;
    e->sigma = xe_sigma;
    e->bound = xe_bound;
    *out = reg(e);
    return HE_OK;
}
int he_encryptor_destroy(he_handle h) { return unreg(h, T_ENCRYPTOR); }
int he_encryptor_set_key(he_handle henc, int kind, const he_handle key[4]) {
    static const char *who = "he_encryptor_set_key";
    GET(e, Encryptor, henc, T_ENCRYPTOR);
    if (kind < 0 || kind > 2 || (kind && !key)) return fail(HE_EINVAL, "%s: kind %d (0 none, 1 sk, 2 pk)", who, kind);
    he_handle k[4] = {0, 0, 0, 0};
    const int n = kind == 1 ? 2 : kind == 2 ? 4 : 0;
    for (int i = 0; i < n; i++) {
        const bool isP = i & 1;
        if (isP && (!e->hp || !key[i])) continue;  // (no special primes: not read; 0 otherwise: refused by the calls that read P)
        auto p = get<Poly>(key[i], T_POLY);  // checkSk / checkPk (:466-479): the ring degree
        if (!p) return fail(HE_EHANDLE, "%s: bad Poly handle for key[%d]", who, i);
        if (p->ctx.get() != &e->ctx() || p->N != e->ev->be->Q->N) return fail(HE_EINVAL, "%s: key[%d] is not a polynomial of the encryptor's rings", who, i);
        k[i] = key[i];
    }
    std::lock_guard<std::mutex> lk(e->mu);
    e->kind = kind;
    std::copy(k, k + 4, e->key);
    return HE_OK;
}

// encryptZeroSkFromC1QP (:406-433); levelP = -1: the ring.Poly form
static int encrypt_zero_sk_from_c1(Encryptor &e, const he_handle *key, int levelQ, int levelP, int is_ntt, int is_montgomery, he_handle c0Q,
                                   he_handle c0P, he_handle c1Q, he_handle c1P) {
    TRY(he_sampler_gaussian_read(e.hq, levelQ, e.prng, e.sigma, e.bound, 0, 0, c0Q));
    if (levelP >= 0) TRY(he_centered_lift(e.hev, 3, c0Q, levelQ + 1, levelQ, c0Q, levelP, c0P));
    TRY(he_ntt(e.hq, levelQ, c0Q, c0Q));
    if (levelP >= 0) TRY(he_ntt(e.hp, levelP, c0P, c0P));
    if (is_montgomery) {
        TRY(he_mform(e.hq, levelQ, c0Q, c0Q));
        if (levelP >= 0) TRY(he_mform(e.hp, levelP, c0P, c0P));
    }
    TRY(he_binop(e.hq, levelQ, HE_MUL_COEFFS_MONTGOMERY_THEN_SUB, c1Q, key[0], c0Q));
    if (levelP >= 0) TRY(he_binop(e.hp, levelP, HE_MUL_COEFFS_MONTGOMERY_THEN_SUB, c1P, key[1], c0P));
    if (!is_ntt) {
        TRY(he_intt(e.hq, levelQ, c0Q, c0Q));
        if (levelP >= 0) TRY(he_intt(e.hp, levelP, c0P, c0P));
        TRY(he_intt(e.hq, levelQ, c1Q, c1Q));
        if (levelP >= 0) TRY(he_intt(e.hp, levelP, c1P, c1P));
    }
    return HE_OK;
}
// encryptZeroSk (:347-393)
static int encrypt_zero_sk(Encryptor &e, const he_handle *key, int levelQ, int levelP, int is_ntt, int is_montgomery, he_handle c0Q,
                           he_handle c0P, he_handle c1Q, he_handle c1P) {
    TRY(he_sampler_uniform_read(e.hq, levelQ, levelP >= 0 ? e.hp : 0, levelP >= 0 ? levelP : 0, e.prng, 0, c1Q, levelP >= 0 ? c1P : 0));
    if (!is_ntt) {
        TRY(he_ntt(e.hq, levelQ, c1Q, c1Q));
        if (levelP >= 0) TRY(he_ntt(e.hp, levelP, c1P, c1P));
    }
    return encrypt_zero_sk_from_c1(e, key, levelQ, levelP, is_ntt, is_montgomery, c0Q, c0P, c1Q, c1P);
}
// encryptZeroPk (:204-299); qp: the Element[ringqp.Poly] form, otherwise ct{0,1}P are the temporaries of the ring.Poly form (levelP 0)
static int encrypt_zero_pk(Encryptor &e, const he_handle *key, int levelQ, int levelP, bool qp, int is_ntt, int is_montgomery, he_handle c0Q,
                           he_handle c0P, he_handle c1Q, he_handle c1P, int B) {
    TmpPoly uQ, uP, t0P, t1P;
    TRY(uQ.alloc(e.hq, levelQ + 1, B));
    TRY(uP.alloc(e.hp, levelP + 1, B));
    if (!qp) {
        TRY(t0P.alloc(e.hp, levelP + 1, B));
        TRY(t1P.alloc(e.hp, levelP + 1, B));
        c0P = t0P.h;
        c1P = t1P.h;
    }
    const he_handle ctQ[2] = {c0Q, c1Q}, ctP[2] = {c0P, c1P};
    TRY(he_sampler_ternary_read(e.hq, levelQ, e.prng, e.xs_p, 0, 0, uQ.h));
    TRY(he_centered_lift(e.hev, 3, uQ.h, levelQ + 1, levelQ, uQ.h, levelP, uP.h));
    TRY(he_ntt(e.hq, levelQ, uQ.h, uQ.h));
    TRY(he_ntt(e.hp, levelP, uP.h, uP.h));
    for (int k = 0; k < 2; k++) {
        TRY(he_mul_coeffs_montgomery(e.hq, levelQ, uQ.h, key[2 * k], ctQ[k]));
        TRY(he_mul_coeffs_montgomery(e.hp, levelP, uP.h, key[2 * k + 1], ctP[k]));
    }
    for (int k = 0; k < 2; k++) {
        TRY(he_intt(e.hq, levelQ, ctQ[k], ctQ[k]));
        TRY(he_intt(e.hp, levelP, ctP[k], ctP[k]));
    }
    for (int k = 0; k < 2; k++) {  // e := u (the buffer)
        TRY(he_sampler_gaussian_read(e.hq, levelQ, e.prng, e.sigma, e.bound, 0, 0, uQ.h));
        TRY(he_centered_lift(e.hev, 3, uQ.h, levelQ + 1, levelQ, uQ.h, levelP, uP.h));
        TRY(he_add(e.hq, levelQ, ctQ[k], uQ.h, ctQ[k]));
        TRY(he_add(e.hp, levelP, ctP[k], uP.h, ctP[k]));
    }
    if (!qp)
        for (int k = 0; k < 2; k++) TRY(he_moddown_qp_to_q(e.hbe, levelQ, levelP, ctQ[k], ctP[k], ctQ[k]));
    if (is_ntt)
        for (int k = 0; k < 2; k++) {
            TRY(he_ntt(e.hq, levelQ, ctQ[k], ctQ[k]));
            if (qp) TRY(he_ntt(e.hp, levelP, ctP[k], ctP[k]));
        }
    if (is_montgomery)
        for (int k = 0; k < 2; k++) {
            TRY(he_mform(e.hq, levelQ, ctQ[k], ctQ[k]));
            if (qp) TRY(he_mform(e.hp, levelP, ctP[k], ctP[k]));
        }
    return HE_OK;
}
// encryptZeroPkNoP (:301-342): the metadata's IsMontgomery is not read there
static int encrypt_zero_pk_nop(Encryptor &e, const he_handle *key, int levelQ, int is_ntt, he_handle c0, he_handle c1, int B) {
    TmpPoly buf;
    TRY(buf.alloc(e.hq, levelQ + 1, B));
    const he_handle ct[2] = {c0, c1};
    TRY(he_sampler_ternary_read(e.hq, levelQ, e.prng, e.xs_p, 0, 0, buf.h));
    TRY(he_ntt(e.hq, levelQ, buf.h, buf.h));
    TRY(he_mul_coeffs_montgomery(e.hq, levelQ, buf.h, key[0], c0));
    TRY(he_mul_coeffs_montgomery(e.hq, levelQ, buf.h, key[2], c1));
    for (int k = 0; k < 2; k++) {
        if (is_ntt) {
            TRY(he_sampler_gaussian_read(e.hq, levelQ, e.prng, e.sigma, e.bound, 0, 0, buf.h));
            TRY(he_ntt(e.hq, levelQ, buf.h, buf.h));
            TRY(he_add(e.hq, levelQ, ct[k], buf.h, ct[k]));
        } else {
            TRY(he_intt(e.hq, levelQ, ct[k], ct[k]));
            TRY(he_sampler_gaussian_read(e.hq, levelQ, e.prng, e.sigma, e.bound, 0, 1, ct[k]));
        }
    }
    return HE_OK;
}
// EncryptZero (:176-188) without the frame; qp: an Element[ringqp.Poly]
static int encrypt_zero(Encryptor &e, const char *who, int levelQ, int levelP, bool qp, int is_ntt, int is_montgomery, he_handle c0Q, he_handle c0P,
                        he_handle c1Q, he_handle c1P, const he_handle *extra, int nextra) {
    int kind;
    he_handle key[4];
    {
        std::lock_guard<std::mutex> lk(e.mu);
        kind = e.kind;
        std::copy(e.key, e.key + 4, key);
    }
    if (kind == 0) return fail(HE_EINVAL, "%s: the encryptor has no encryption key", who);
    const bool needP = e.hp && (kind == 2 || (qp && levelP >= 0));  // (encryptZeroPk lifts to P for a ring.Poly element too)
    if (needP && (!key[1] || (kind == 2 && !key[3]))) return fail(HE_EINVAL, "%s: the key was bound without its P part, which this call reads", who);
    if (levelQ < 0 || levelQ > e.maxQ()) return fail(HE_EINVAL, "%s: level %d, the ring has levels 0..%d", who, levelQ, e.maxQ());
    if (qp && kind == 1 && levelP == -1) qp = false;  // a ringqp.Poly without a P part (GenPublicKey without special primes): c0P, c1P are not read
    if (qp && (!e.hp || levelP < 0 || levelP > e.maxP())) return fail(HE_EINVAL, "%s: levelP %d, ringP has levels 0..%d", who, levelP, e.maxP());
    int B = 0;
    TRY(batch_of(c0Q, who, &B));
    const he_handle outs[4] = {c0Q, c1Q, qp ? c0P : 0, qp ? c1P : 0};
    he_handle others[8] = {key[0], key[1], key[2], key[3], 0, 0, 0, 0};
    for (int i = 0; i < nextra && i < 4; i++) others[4 + i] = extra[i];
    TRY(rlwe_distinct(who, outs, 4, others, 8));
    if (kind == 1) return encrypt_zero_sk(e, key, levelQ, qp ? levelP : -1, is_ntt, is_montgomery, c0Q, c0P, c1Q, c1P);
    if (!qp && !e.hp) return encrypt_zero_pk_nop(e, key, levelQ, is_ntt, c0Q, c1Q, B);
    return encrypt_zero_pk(e, key, levelQ, qp ? levelP : 0, qp, is_ntt, is_montgomery, c0Q, c0P, c1Q, c1P, B);
}
int he_encrypt_zero(he_handle henc, int level, int is_ntt, int is_montgomery, he_handle c0, he_handle c1) {
    static const char *who = "he_encrypt_zero";
    GET(e, Encryptor, henc, T_ENCRYPTOR);
    TRY(rlwe_frame_begin(e->ctx(), who));
    const int rc = encrypt_zero(*e, who, level, -1, false, is_ntt, is_montgomery, c0, 0, c1, 0, nullptr, 0);
    const int rs = rlwe_frame_end(e->ctx());
    return rc != HE_OK ? rc : rs;
}
int he_encrypt_zero_qp(he_handle henc, int levelQ, int levelP, int is_ntt, int is_montgomery, he_handle c0Q, he_handle c0P, he_handle c1Q,
                       he_handle c1P) {
    static const char *who = "he_encrypt_zero_qp";
    GET(e, Encryptor, henc, T_ENCRYPTOR);
    TRY(rlwe_frame_begin(e->ctx(), who));
    const int rc = encrypt_zero(*e, who, levelQ, levelP, true, is_ntt, is_montgomery, c0Q, c0P, c1Q, c1P, nullptr, 0);
    const int rs = rlwe_frame_end(e->ctx());
    return rc != HE_OK ? rc : rs;
}
// addPtToCt (:481-507) without the frame
static int add_pt_to_ct(Encryptor &e, const char *who, int level, int pt_is_ntt, int ct_is_ntt, he_handle pt, he_handle c0) {
    if (level < 0 || level > e.maxQ()) return fail(HE_EINVAL, "%s: level %d, the ring has levels 0..%d", who, level, e.maxQ());
    TRY(rlwe_distinct(who, &c0, 1, &pt, 1));
    if (!pt_is_ntt == !ct_is_ntt) return he_add(e.hq, level, c0, pt, c0);
    int B = 0;
    TRY(batch_of(pt, who, &B));
    TmpPoly buf;
    TRY(buf.alloc(e.hq, level + 1, B));
    if (pt_is_ntt) TRY(he_ntt(e.hq, level, pt, buf.h));  // (:493, as the reference writes it)
    else TRY(he_intt(e.hq, level, pt, buf.h));           // (:500)
    return he_add(e.hq, level, c0, buf.h, c0);
}
int he_add_pt_to_ct(he_handle henc, int level, int pt_is_ntt, int ct_is_ntt, he_handle pt, he_handle c0) {
    static const char *who = "he_add_pt_to_ct";
    GET(e, Encryptor, henc, T_ENCRYPTOR);
    TRY(rlwe_frame_begin(e->ctx(), who));
    const int rc = add_pt_to_ct(*e, who, level, pt_is_ntt, ct_is_ntt, pt, c0);
    const int rs = rlwe_frame_end(e->ctx());
    return rc != HE_OK ? rc : rs;
}
int he_encrypt(he_handle henc, int pt_level, int ct_level, int is_ntt, int is_montgomery, he_handle pt, he_handle c0, he_handle c1, int *level_out) {
    static const char *who = "he_encrypt";
    GET(e, Encryptor, henc, T_ENCRYPTOR);
    TRY(rlwe_frame_begin(e->ctx(), who));
    const int level = std::min(pt_level, ct_level);  // (:141)
    if (level_out) *level_out = level;
    if (!get<Poly>(pt, T_POLY)) return fail(HE_EHANDLE, "%s: bad Poly handle for the plaintext", who);
    int rc = encrypt_zero(*e, who, level, -1, false, is_ntt, is_montgomery, c0, 0, c1, 0, &pt, 1);
    if (rc == HE_OK) rc = add_pt_to_ct(*e, who, level, is_ntt, is_ntt, pt, c0);
    const int rs = rlwe_frame_end(e->ctx());
    return rc != HE_OK ? rc : rs;
}

int he_decryptor_create(he_handle hev, he_handle skQ, he_handle *out) {
    static const char *who = "he_decryptor_create";
    GET(ev, Evaluator, hev, T_EVAL);
    if (!out) return fail(HE_EINVAL, "%s: null output", who);
    auto p = get<Poly>(skQ, T_POLY);
    if (!p) return fail(HE_EHANDLE, "%s: bad Poly handle for skQ", who);
    if (p->ctx != ev->be->ctx || p->N != ev->be->Q->N) return fail(HE_EINVAL, "%s: skQ is not a polynomial of the evaluator's ringQ", who);
    auto d = std::make_shared<Decryptor>();
    d->bind(ev);
    d->sk = skQ;
    *out = reg(d);
    return HE_OK;
}
int he_decryptor_destroy(he_handle h) { return unreg(h, T_DECRYPTOR); }
static int decrypt(Decryptor &d, const char *who, int level, int is_ntt, int degree, const he_handle *ct, he_handle pt) {
    if (is_ntt) TRY(he_poly_copy(pt, ct[degree], level));  // (:61-65)
    else TRY(he_ntt_lazy(d.hq, level, ct[degree], pt));
    TmpPoly buf;
    if (!is_ntt && degree > 0) {
        int B = 0;
        TRY(batch_of(pt, who, &B));
        TRY(buf.alloc(d.hq, level + 1, B));
    }
    for (int i = degree; i > 0; i--) {  // (:67-84)
        TRY(he_mul_coeffs_montgomery(d.hq, level, pt, d.sk, pt));
        if (!is_ntt) {
            TRY(he_ntt_lazy(d.hq, level, ct[i - 1], buf.h));
            TRY(he_add(d.hq, level, pt, buf.h, pt));
        } else {
            TRY(he_add(d.hq, level, pt, ct[i - 1], pt));
        }
        if ((i & 7) == 7) TRY(he_reduce(d.hq, level, pt, pt));
    }
    // (:86: no Reduce when degree & 7 == 7.  For a coefficient-domain ciphertext the reference's INTT then reads the unreduced sum of
    // NTTLazy words, up to 7q, on which its butterflies are not exact: its words there are not the decryption.  he_ntt_lazy keeps
    // [0, 2q) and he_intt takes canonical words, so the Reduce is made in that case too and the result is the canonical decryption)
    if ((degree & 7) != 7 || !is_ntt) TRY(he_reduce(d.hq, level, pt, pt));
    if (!is_ntt) TRY(he_intt(d.hq, level, pt, pt));
    return HE_OK;
}
int he_decryptor_decrypt(he_handle hdec, int ct_level, int pt_level, int is_ntt, int degree, const he_handle *ct, he_handle pt, int *level_out) {
    static const char *who = "he_decryptor_decrypt";
    GET(d, Decryptor, hdec, T_DECRYPTOR);
    TRY(rlwe_frame_begin(d->ctx(), who));
    if (!ct || degree < 0 || degree > 63) return fail(HE_EINVAL, "%s: degree %d is not in [0, 63]", who, degree);
    const int level = std::min(ct_level, pt_level);  // (:53)
    if (level < 0 || level > d->maxQ()) return fail(HE_EINVAL, "%s: level %d, the ring has levels 0..%d", who, level, d->maxQ());
    if (level_out) *level_out = level;
    he_handle others[65];
    for (int i = 0; i <= degree; i++) others[i] = ct[i];
    others[degree + 1] = d->sk;
    TRY(rlwe_distinct(who, &pt, 1, others, degree + 2));
    const int rc = decrypt(*d, who, level, is_ntt, degree, ct, pt);
    const int rs = rlwe_frame_end(d->ctx());
    return rc != HE_OK ? rc : rs;
}

// ---------------------------------------------------------------------------------------
// rlwe.KeyGenerator (include/hering_keygen.h; core/rlwe/keygenerator.go).  The secret keys, the relinearization key and the Galois
// keys are compositions in front of keygen_evaluation_key, which draws row by row into the key's own storage and then finishes
// every row at once (launch_evk_finish).
// ---------------------------------------------------------------------------------------
struct KeyGen : Obj, RlweFrame {
    std::shared_ptr<Prng> prng_keep;
    he_handle prng = 0;
    double xs_p = 0, sigma = 0, bound = 0;
    KeyGen() : Obj(T_KEYGEN) {}
    ~KeyGen() override {
        if (prng) reg_drop(prng);
    }
};
int he_keygen_create(he_handle hev, he_handle hprng, double xs_p, double xe_sigma, double xe_bound, he_handle *out) {
    static const char *who = "he_keygen_create";
    GET(ev, Evaluator, hev, T_EVAL);
    GET(g, Prng, hprng, T_PRNG);
    if (!out) return fail(HE_EINVAL, "%s: null output", who);
    TRY(ternary_density(xs_p, who));
    if (!(xe_sigma > 0.0) || xe_sigma > 0x1p53 || !(xe_bound >= 0.0) || xe_bound > 0x1p62)
        return fail(HE_EINVAL, "%s: Xe = {%g, %g}: sigma in (0, 2^53] and bound in [0, 2^62] (hering_sampler.h)", who, xe_sigma, xe_bound);
    auto k = std::make_shared<KeyGen>();
    k->bind(ev);
    k->prng_keep = g;
    k->prng = reg(g);
    k->xs_p = xs_p;
    k->sigma = xe_sigma;
    k->bound = xe_bound;
    *out = reg(k);
    return HE_OK;
}
int he_keygen_destroy(he_handle h) { return unreg(h, T_KEYGEN); }

// sampleSparse (ring/sampler_ternary.go:198-263).  The walk is sequential over bytes that are on the host: it is made here, into
// the indices of matrixValues per coefficient, which one launch of the ternary expansion then writes into every limb.
int he_keygen_ternary_sparse_read(he_handle hr, int level, he_handle hg, int hw, int montgomery, he_handle hpol) {
    static const char *who = "he_keygen_ternary_sparse_read";
    GET(r, Ring, hr, T_RING);
    GET(g, Prng, hg, T_PRNG);
    std::shared_ptr<Poly> pol;
    TRY(sampler_poly(*r, level, hpol, 1, "pol", who, &pol));
    if (hw <= 0) return fail(HE_EINVAL, "%s: a Hamming weight of %d", who, hw);
    Ctx &c = *r->ctx;
    if (c.capturing) return fail(HE_EINVAL, "%s: host transfers cannot be captured in a graph", who);
    const int N = r->N;
    if (hw > N) hw = N;  // :202-204
    uint64_t lut1[kMaxLimbs], lut2[kMaxLimbs];  // matrixValues[k][1], [2] (:82-104)
    for (int i = 0; i <= level; i++) {
        const uint64_t q = r->moduli[i];
        lut1[i] = montgomery ? to_mont(1, q) : 1;
        lut2[i] = montgomery ? to_mont(q - 1, q) : q - 1;
    }
    std::lock_guard<std::mutex> lk(g->mu);
    const size_t nsign = ((size_t)hw + 7) / 8, expected = nsign + 4 * (size_t)hw, cap = expected * 64;
    std::vector<uint64_t> vals((size_t)N, 0);
    std::vector<uint32_t> index((size_t)N);
    for (int i = 0; i < N; i++) index[(size_t)i] = (uint32_t)i;
    auto wipe_host = [&]() {
        Prng::wipe(vals.data(), vals.size() * 8);
        Prng::wipe(index.data(), index.size() * 4);
    };
    size_t off = nsign;  // :216-222: the sign bytes first
    int rc = g->fetch(expected + expected / 2, who);
    for (int i = 0; i < hw && rc == HE_OK; i++) {
        const uint32_t left = (uint32_t)(N - i);
        const uint32_t mask = (uint32_t)(((uint64_t)1 << (64 - __builtin_clzll((uint64_t)left))) - 1);  // :230
        uint32_t j;
        do {  // randInt32 (:232-236): four bytes, big-endian, masked
            if (off + 4 > g->buf.size()) {
                const size_t want = std::max(off + 4, g->buf.size() * 2);
                if (want > cap) rc = fail(HE_EPRNG, "%s: the source did not let the call finish within %zu bytes (64 times the expected %zu)", who, cap, expected);
                else rc = g->fetch(want, who);
                if (rc != HE_OK) break;
            }
            const uint8_t *b = g->buf.data() + off;
            j = (((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | (uint32_t)b[3]) & mask;
            off += 4;
        } while (j >= left);
        if (rc != HE_OK) break;
        const uint64_t coeff = (g->buf[(size_t)i >> 3] >> (i & 7)) & 1;  // :238 (0: +1, 1: -1)
        vals[index[j]] = coeff + 1;                                        // :240-244
        index[j] = index[left - 1];                                        // :247-248
    }
    if (rc != HE_OK) {
        wipe_host();
        return rc;
    }
    {
        Scope sc(&c);
        if ((rc = c.arena_reserve((size_t)N + 8)) != HE_OK) {
            wipe_host();
            return rc;
        }
        uint64_t *d_vals = c.arena_take((size_t)N);
        HIP_TRY(hipMemcpyAsync(d_vals, vals.data(), (size_t)N * 8, hipMemcpyHostToDevice, c.stream));
        HIP_TRY(launch_sampler_expand(r->dev.mc, d_vals, false, false, false, lut1, lut2, pol->view(), N, level + 1, 1, c.stream));
        HIP_TRY(hipMemsetAsync(d_vals, 0, (size_t)N * 8, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
    }
    wipe_host();
    g->consume(off);
    return HE_OK;
}

// a secret-key operand or output: a polynomial of the generator's context and degree with `limbs` limbs, batch 1
static int keygen_poly(const KeyGen &k, const char *who, he_handle h, int limbs, const char *name, std::shared_ptr<Poly> *out) {
    auto p = get<Poly>(h, T_POLY);
    if (!p) return fail(HE_EHANDLE, "%s: bad Poly handle for %s", who, name);
    if (p->ctx.get() != &k.ctx() || p->N != k.ev->be->Q->N) return fail(HE_EINVAL, "%s: %s is not a polynomial of the generator's rings", who, name);
    if (p->nlimbs < limbs) return fail(HE_EINVAL, "%s: %s has %d limbs, %d needed", who, name, p->nlimbs, limbs);
    if (p->batch != 1) return fail(HE_EINVAL, "%s: %s has %d entries; a secret key is one polynomial", who, name, p->batch);
    if (out) *out = p;
    return HE_OK;
}
static int keygen_sk_levels(const KeyGen &k, const char *who, int levelQ, int levelP, he_handle skQ, he_handle skP) {
    if (levelQ < 0 || levelQ > k.maxQ()) return fail(HE_EINVAL, "%s: levelQ %d, the ring has levels 0..%d", who, levelQ, k.maxQ());
    if (levelP < -1 || levelP > k.maxP()) return fail(HE_EINVAL, "%s: levelP %d, ringP has levels -1..%d", who, levelP, k.maxP());
    TRY(keygen_poly(k, who, skQ, levelQ + 1, "skQ", nullptr));
    if (levelP >= 0) {
        TRY(keygen_poly(k, who, skP, levelP + 1, "skP", nullptr));
        TRY(rlwe_distinct(who, &skQ, 1, &skP, 1));
    }
    return HE_OK;
}
// genSecretKeyFromSampler (:64-69) after the Read
static int keygen_sk_finish(KeyGen &k, int levelQ, int levelP, he_handle skQ, he_handle skP) {
    if (levelP >= 0) TRY(he_centered_lift(k.hev, 3, skQ, levelQ + 1, levelQ, skQ, levelP, skP));
    TRY(he_ntt(k.hq, levelQ, skQ, skQ));
    if (levelP >= 0) TRY(he_ntt(k.hp, levelP, skP, skP));
    TRY(he_mform(k.hq, levelQ, skQ, skQ));
    if (levelP >= 0) TRY(he_mform(k.hp, levelP, skP, skP));
    return HE_OK;
}
int he_keygen_secret_key(he_handle hk, int levelQ, int levelP, he_handle skQ, he_handle skP) {
    static const char *who = "he_keygen_secret_key";
    GET(k, KeyGen, hk, T_KEYGEN);
    TRY(rlwe_frame_begin(k->ctx(), who));
    TRY(keygen_sk_levels(*k, who, levelQ, levelP, skQ, skP));
    int rc = he_sampler_ternary_read(k->hq, levelQ, k->prng, k->xs_p, 0, 0, skQ);  // :62
    if (rc == HE_OK) rc = keygen_sk_finish(*k, levelQ, levelP, skQ, skP);
    const int rs = rlwe_frame_end(k->ctx());
    return rc != HE_OK ? rc : rs;
}
int he_keygen_secret_key_hw(he_handle hk, int hw, int levelQ, int levelP, he_handle skQ, he_handle skP) {
    static const char *who = "he_keygen_secret_key_hw";
    GET(k, KeyGen, hk, T_KEYGEN);
    TRY(rlwe_frame_begin(k->ctx(), who));
    if (hw <= 0) return fail(HE_EINVAL, "%s: a Hamming weight of %d", who, hw);
    TRY(keygen_sk_levels(*k, who, levelQ, levelP, skQ, skP));
    int rc = he_keygen_ternary_sparse_read(k->hq, levelQ, k->prng, hw, 0, skQ);  // :50, montgomery = false
    if (rc == HE_OK) rc = keygen_sk_finish(*k, levelQ, levelP, skQ, skP);
    const int rs = rlwe_frame_end(k->ctx());
    return rc != HE_OK ? rc : rs;
}

// The gadget vector of a key, row by row: G[row][index] = MForm(P 2^(j pw2) mod q_index) on the Q limbs of the row's digit
// (gadgetciphertext.go:183-237), 0 elsewhere.  P: the product of the key's special primes (1 without).  mont = false: P 2^(j pw2) mod
// q_index itself (round one of the relinearization protocol, include/hering_multiparty.h).
static std::vector<uint64_t> gadget_table(const Evk &k, bool mont = true) {
    const BasisExtender &be = *k.ev->be;
    const int nQk = k.nQk, alpha = std::max(k.nPk, 1), nrns = k.pw2 ? (int)k.nj.size() : k.beta;
    std::vector<uint64_t> G((size_t)k.beta * nQk, 0);
    for (int i = 0; i < nrns; i++) {
        const int nji = k.pw2 ? k.nj[(size_t)i] : 1;
        for (int j = 0; j < nji; j++) {
            const int row = k.pw2 ? k.prefix[(size_t)i] + j : i;
            for (int kk = 0; kk < alpha; kk++) {
                const int index = i * alpha + kk;
                if (index >= nQk) break;  // (:218: #pj does not divide #qi)
                const uint64_t q = be.Q->moduli[(size_t)index];
                uint64_t f = 1 % q;
                for (int t = 0; t < k.nPk; t++) f = mulmod(f, be.P->moduli[(size_t)t] % q, q);
                for (int t = 0; t < j; t++) f = mulmod(f, ((uint64_t)1 << k.pw2) % q, q);  // (:237, once per window)
                G[(size_t)row * nQk + index] = mont ? to_mont(f, q) : f;
            }
        }
    }
    return G;
}
static int evk_shape_for_keygen(const Evk &k, const char *who, const char *name) {
    if (!k.pw2 && k.beta != base_rns_size(k.nQk - 1, k.nPk - 1))
        return fail(HE_EINVAL, "%s: %s has %d digits; a key at levels (%d, %d) has %d", who, name, k.beta, k.nQk - 1, k.nPk - 1, base_rns_size(k.nQk - 1, k.nPk - 1));
    if (k.pw2 && (int)k.nj.size() != k.nQk) return fail(HE_EINVAL, "%s: %s: one RNS digit per key Q-limb is required", who, name);
    if (k.nQk + k.nPk > kMaxLimbs) return fail(HE_EINVAL, "%s: %s has %d limbs per row, at most %d", who, name, k.nQk + k.nPk, kMaxLimbs);
    return HE_OK;
}
static void evk_rows_args(const Evk &k, EvkRowsArgs &a) {
    const BasisExtender &be = *k.ev->be;
    a.key = k.d;
    a.c1 = k.d;
    a.blk = (size_t)(k.nQk + k.nPk) * be.Q->N;
    a.N = be.Q->N; a.rows = k.beta; a.nq = k.nQk; a.np = k.nPk;
    a.mc = be.qp.mc;
    for (int i = 0; i < k.nQk; i++) a.mod[i] = (uint8_t)i;
    for (int i = 0; i < k.nPk; i++) a.mod[k.nQk + i] = (uint8_t)(be.LQ + i);
}
// the gadget table of k in scratch (the caller holds the context and has reserved beta nQk + 2 words more)
// (G is the caller's: it outlives the copy, which the caller's drain of the stream ends)
static int gadget_table_upload(Ctx &c, const Evk &k, std::vector<uint64_t> &G, const uint64_t **d_G, bool mont = true) {
    G = gadget_table(k, mont);
    uint64_t *p = c.arena_take(G.size());
    HIP_TRY(hipMemcpyAsync(p, G.data(), G.size() * 8, hipMemcpyHostToDevice, c.stream));
    *d_G = p;
    return HE_OK;
}
int he_gadget_add_poly(he_handle hpt, he_handle hk0, he_handle hk1) {
    static const char *who = "he_gadget_add_poly";
    GET(k0, Evk, hk0, T_EVK);
    std::shared_ptr<Evk> k1;
    if (hk1) {
        k1 = get<Evk>(hk1, T_EVK);
        if (!k1) return fail(HE_EHANDLE, "%s: bad Evk handle for evk1", who);
        if (k1 == k0) return fail(HE_EINVAL, "%s: evk0 and evk1 are one key", who);
        if (k1->ev != k0->ev || k1->beta != k0->beta || k1->nQk != k0->nQk || k1->nPk != k0->nPk || k1->pw2 != k0->pw2 || k1->nj != k0->nj)
            return fail(HE_EINVAL, "%s: evk0 and evk1 differ in evaluator or shape", who);
    }
    TRY(evk_shape_for_keygen(*k0, who, "evk0"));
    BasisExtender &be = *k0->ev->be;
    Ctx &c = *be.ctx;
    auto pt = get<Poly>(hpt, T_POLY);
    if (!pt) return fail(HE_EHANDLE, "%s: bad Poly handle for pt", who);
    if (pt->ctx != be.ctx || pt->N != be.Q->N || pt->nlimbs < k0->nQk || pt->batch != 1)
        return fail(HE_EINVAL, "%s: pt must be one polynomial of the key's ringQ with %d limbs", who, k0->nQk);
    if (c.capturing) return fail(HE_EINVAL, "%s: not inside a graph capture", who);
    Scope sc(&c);
    TRY(c.arena_reserve((size_t)k0->beta * k0->nQk + 8));
    EvkRowsArgs a;
    evk_rows_args(*k0, a);
    a.pt = pt->d;
    std::vector<uint64_t> G;
    TRY(gadget_table_upload(c, *k0, G, &a.G));
    for (int u = 0; u < (k1 ? 2 : 1); u++) {  // `for u, ct := range cts` (:225): component u of key u
        Evk &k = u ? *k1 : *k0;
        a.key = k.d;
        a.comp = u;
        HIP_TRY(launch_gadget_add(a, c.stream));
        TRY(evk_derive(k));
    }
    HIP_TRY(hipStreamSynchronize(c.stream));
    return HE_OK;
}

// genEvaluationKey (:287-330) without the frame.  skIn (nQk limbs), skOut = (skOutQ, skOutP): device words, NTT and Montgomery.
// crp: EvaluationKeyGenProtocol.GenShare (multiparty/keygen_evk.go:86-183; include/hering_multiparty.h) instead -- no uniform draw, c1
// is component 1 of crp (a key of k's shape, possibly k), the Gaussians are drawn j outer and i inner, and k, a share, is not committed.
static int keygen_evaluation_key(KeyGen &kg, const char *who, const uint64_t *skIn, const uint64_t *skOutQ, const uint64_t *skOutP, Evk &k,
                                 const Evk *crp = nullptr) {
    BasisExtender &be = *kg.ev->be;
    Ctx &c = *be.ctx;
    Prng &g = *kg.prng_keep;
    const int N = be.Q->N, R = k.beta, nQk = k.nQk, nPk = k.nPk;
    const size_t blk = (size_t)(nQk + nPk) * N;
    // the small values of every row's Gaussian, [R][N]: outside the arena, which every draw resets
    const size_t stage_bytes = (size_t)R * N * 8;
    uint64_t *d_e = nullptr;
    {
        Scope sc(&c);
        HIP_TRY(c.pool_take(stage_bytes, (void **)&d_e));
    }
    int rc = HE_OK;
    const ModConst *const mc[2] = {be.Q->dev.mc, nPk ? be.P->dev.mc : nullptr};
    const int nl[2] = {nQk, nPk};
    const size_t bs[2] = {2 * blk, 2 * blk};
    std::vector<int> order;  // the rows in drawing order
    if (crp && k.pw2) {      // (keygen_evk.go:134-138)
        const int nmax = *std::max_element(k.nj.begin(), k.nj.end());
        for (int j = 0; j < nmax; j++)
            for (size_t i = 0; i < k.nj.size(); i++)
                if (j < k.nj[i]) order.push_back(k.prefix[i] + j);
    } else {
        for (int r = 0; r < R; r++) order.push_back(r);
    }
    for (size_t t = 0; t < order.size() && rc == HE_OK; t++) {  // one encryptZeroSk per row (:309-320): the uniform c1 (Q, then P), then the Gaussian e
        const int r = order[t];
        if (!crp) {
            uint64_t *c1 = k.d + ((size_t)2 * r + 1) * blk;
            uint64_t *const out[2] = {c1, c1 + (size_t)nQk * N};
            rc = uniform_read_run(who, c, g, N, 1, nPk ? 2 : 1, mc, nl, out, bs, false, nullptr);
            if (rc != HE_OK) break;
        }
        rc = gaussian_parse_run(who, c, g, N, 1, kg.sigma, kg.bound, [&](const uint64_t *vals) -> int {
            HIP_TRY(hipMemcpyAsync(d_e + (size_t)r * N, vals, (size_t)N * 8, hipMemcpyDeviceToDevice, c.stream));
            return HE_OK;
        });
    }
    Scope sc(&c);
    std::vector<uint64_t> G;
    if (rc == HE_OK) rc = [&]() -> int {
        TRY(c.arena_reserve((size_t)R * nQk + 8));
        const View c0{k.d, 2 * blk};
        // encryptor.go:411-414: the Gaussian words on the Q limbs and their centred copies on the P limbs, every row at once
        HIP_TRY(launch_sampler_expand(be.qp.mc, d_e, true, false, false, nullptr, nullptr, c0, N, nQk, R, c.stream));
        if (nPk)
            HIP_TRY(launch_sampler_expand(be.qp.mc + be.LQ, d_e, true, false, false, nullptr, nullptr, View{k.d + (size_t)nQk * N, 2 * blk}, N, nPk, R, c.stream));
        LimbTab tab = ident_tab(nQk + nPk);
        for (int i = 0; i < nPk; i++) tab.mod[nQk + i] = (uint8_t)(be.LQ + i);
        HIP_TRY(be_ntt(be, tab, c0, c0, R, false, NTT_REDUCE_INPUT));  // :416-418
        EvkRowsArgs a;
        evk_rows_args(k, a);
        a.skOutQ = skOutQ; a.skOutP = skOutP; a.pt = skIn;
        if (crp) a.c1 = crp->d;
        TRY(gadget_table_upload(c, k, G, &a.G));
        c.acct(3.0 * (nQk + nPk), 0, R, N);
        HIP_TRY(launch_evk_finish(a, c.stream));  // :420-425 and AddPolyTimesGadgetVectorToGadgetCiphertext (:326)
        if (!crp) {
            TRY(evk_derive(k));
            k.word_mul = 1;
        }
        return HE_OK;
    }();
    (void)hipMemsetAsync(d_e, 0, stage_bytes, c.stream);
    HIP_TRY(hipStreamSynchronize(c.stream));
    c.pool_give(stage_bytes, d_e);
    return rc;
}
// the key operand of a generation call: a key of the generator's evaluator with a shape genEvaluationKey serves
static int keygen_evk(const KeyGen &kg, const char *who, he_handle h, std::shared_ptr<Evk> *out) {
    auto k = get<Evk>(h, T_EVK);
    if (!k) return fail(HE_EHANDLE, "%s: bad Evk handle %llu", who, (unsigned long long)h);
    if (k->ev != kg.ev) return fail(HE_EINVAL, "%s: the key belongs to another evaluator than the generator", who);
    TRY(evk_shape_for_keygen(*k, who, "the key"));
    *out = k;
    return HE_OK;
}
// sk = (skQ, skP) at the levels of key k
static int keygen_sk_for(const KeyGen &kg, const char *who, const Evk &k, he_handle skQ, he_handle skP, const char *nameQ, const char *nameP,
                         std::shared_ptr<Poly> *q, std::shared_ptr<Poly> *p) {
    TRY(keygen_poly(kg, who, skQ, k.nQk, nameQ, q));
    if (k.nPk) TRY(keygen_poly(kg, who, skP, k.nPk, nameP, p));
    return HE_OK;
}
int he_keygen_evaluation_key(he_handle hk, he_handle skInQ, he_handle skOutQ, he_handle skOutP, he_handle hevk) {
    static const char *who = "he_keygen_evaluation_key";
    GET(kg, KeyGen, hk, T_KEYGEN);
    TRY(rlwe_frame_begin(kg->ctx(), who));
    std::shared_ptr<Evk> k;
    TRY(keygen_evk(*kg, who, hevk, &k));
    std::shared_ptr<Poly> in, oq, op;
    TRY(keygen_poly(*kg, who, skInQ, k->nQk, "skInQ", &in));
    TRY(keygen_sk_for(*kg, who, *k, skOutQ, skOutP, "skOutQ", "skOutP", &oq, &op));
    { Scope sc(&kg->ctx()); }  // (after the calling thread's queued requests)
    return keygen_evaluation_key(*kg, who, in->d, oq->d, op ? op->d : nullptr, *k);
}
// GenEvaluationKey (:261-285): the two secret keys may live in rings of a smaller degree and at other levels
int he_keygen_evaluation_key_sk(he_handle hk, he_handle skInQ, he_handle skOutQ, he_handle hevk) {
    static const char *who = "he_keygen_evaluation_key_sk";
    GET(kg, KeyGen, hk, T_KEYGEN);
    TRY(rlwe_frame_begin(kg->ctx(), who));
    std::shared_ptr<Evk> k;
    TRY(keygen_evk(*kg, who, hevk, &k));
    auto in = get<Poly>(skInQ, T_POLY), out = get<Poly>(skOutQ, T_POLY);
    if (!in || !out) return fail(HE_EHANDLE, "%s: bad Poly handle for %s", who, in ? "skOutQ" : "skInQ");
    const int N = kg->ev->be->Q->N;
    for (const auto &p : {in, out})
        if (p->ctx.get() != &kg->ctx() || p->batch != 1 || p->N > N || p->N < 16 || (p->N & (p->N - 1)))
            return fail(HE_EINVAL, "%s: a secret key is one polynomial of the generator's context, of a degree in [16, %d]", who, N);
    const int lin = std::min(in->nlimbs, kg->maxQ() + 1) - 1, lout = std::min(out->nlimbs, kg->maxQ() + 1) - 1;
    if (lout < k->nQk - 1) return fail(HE_EINVAL, "%s: skOutQ has %d limbs, the key's levelQ needs %d", who, out->nlimbs, k->nQk);
    const int levelP = k->nPk - 1;
    TmpPoly bOutQ, bOutP, bIn, b0;
    int rc = bOutQ.alloc(kg->hq, lout + 1, 1);
    if (rc == HE_OK) rc = bIn.alloc(kg->hq, lout + 1, 1);
    if (rc == HE_OK) rc = b0.alloc(kg->hq, 1, 1);
    if (rc == HE_OK && levelP >= 0) rc = bOutP.alloc(kg->hp, levelP + 1, 1);
    if (rc == HE_OK) rc = he_map_small_to_large_ntt(skOutQ, bOutQ.h, lout);  // :271
    if (rc == HE_OK && levelP >= 0) {  // :276-278, ExtendBasisSmallNormAndCenterNTTMontgomery (utils.go:250-284) into P
        rc = he_intt(kg->hq, 0, bOutQ.h, b0.h);
        if (rc == HE_OK) rc = he_imform(kg->hq, 0, b0.h, b0.h);
        if (rc == HE_OK) rc = he_centered_lift(kg->hev, 3, b0.h, 1, 0, b0.h, levelP, bOutP.h);
        if (rc == HE_OK) rc = he_ntt(kg->hp, levelP, bOutP.h, bOutP.h);
        if (rc == HE_OK) rc = he_mform(kg->hp, levelP, bOutP.h, bOutP.h);
    }
    if (rc == HE_OK) rc = he_map_small_to_large_ntt(skInQ, bIn.h, lin);  // :281
    if (rc == HE_OK) rc = he_intt(kg->hq, 0, bIn.h, bIn.h);              // :282: limbs 0..lout of skIn from its limb 0
    if (rc == HE_OK) rc = he_imform(kg->hq, 0, bIn.h, bIn.h);
    if (rc == HE_OK) rc = he_centered_lift(kg->hev, 3, bIn.h, 1, lout, bIn.h, -1, 0);
    if (rc == HE_OK) rc = he_ntt(kg->hq, lout, bIn.h, bIn.h);
    if (rc == HE_OK) rc = he_mform(kg->hq, lout, bIn.h, bIn.h);
    if (rc == HE_OK) {
        { Scope sc(&kg->ctx()); }
        rc = keygen_evaluation_key(*kg, who, get<Poly>(bIn.h, T_POLY)->d, get<Poly>(bOutQ.h, T_POLY)->d, levelP >= 0 ? get<Poly>(bOutP.h, T_POLY)->d : nullptr, *k);  // :284
    }
    const int rs = rlwe_frame_end(kg->ctx());
    return rc != HE_OK ? rc : rs;
}
int he_keygen_relinearization_key(he_handle hk, he_handle skQ, he_handle skP, he_handle hrlk) {
    static const char *who = "he_keygen_relinearization_key";
    GET(kg, KeyGen, hk, T_KEYGEN);
    TRY(rlwe_frame_begin(kg->ctx(), who));
    std::shared_ptr<Evk> k;
    TRY(keygen_evk(*kg, who, hrlk, &k));
    std::shared_ptr<Poly> q, p;
    TRY(keygen_sk_for(*kg, who, *k, skQ, skP, "skQ", "skP", &q, &p));
    TmpPoly sk2;  // (:114-118; cleared before it goes back to the pool)
    TRY(sk2.alloc(kg->hq, k->nQk, 1));
    int rc = he_mul_coeffs_montgomery(kg->hq, k->nQk - 1, skQ, skQ, sk2.h);
    if (rc == HE_OK) {
        { Scope sc(&kg->ctx()); }
        rc = keygen_evaluation_key(*kg, who, get<Poly>(sk2.h, T_POLY)->d, q->d, p ? p->d : nullptr, *k);
    }
    const int rs = rlwe_frame_end(kg->ctx());
    return rc != HE_OK ? rc : rs;
}
static int evk_same_shape(const char *who, const Evk &a, const Evk &b, const char *na, const char *nb) {
    if (a.ev != b.ev || a.beta != b.beta || a.nQk != b.nQk || a.nPk != b.nPk || a.pw2 != b.pw2 || a.nj != b.nj)
        return fail(HE_EINVAL, "%s: %s and %s differ in evaluator or shape", who, na, nb);
    return HE_OK;
}
// GenGaloisKey (:140-177) without the frame; hcrp: GaloisKeyGenProtocol.GenShare (multiparty/keygen_gal.go:48-71) into the share hgk
static int keygen_galois_key(KeyGen &kg, const char *who, uint64_t gal, he_handle skQ, he_handle skP, he_handle hgk, he_handle hcrp = 0) {
    if (!(gal & 1)) return fail(HE_EINVAL, "%s: the Galois element %llu is even", who, (unsigned long long)gal);
    std::shared_ptr<Evk> k, crp;
    TRY(keygen_evk(kg, who, hgk, &k));
    if (hcrp) {
        TRY(keygen_evk(kg, who, hcrp, &crp));
        TRY(evk_same_shape(who, *crp, *k, "crp", "share"));
    }
    std::shared_ptr<Poly> q, p;
    TRY(keygen_sk_for(kg, who, *k, skQ, skP, "skQ", "skP", &q, &p));
    const Ring &Q = *kg.ev->be->Q;
    gal = reduce_gal(gal, Q.logN, Q.type);
    // a conjugate-invariant ring has the automorphisms 5^k alone: for -5^k (3 modulo 4) AutomorphismNTTIndex(N, 4N, .) holds
    // positions in [N, 2N), an index panic in the reference's AutomorphismNTTWithIndex
    if (Q.type == 1 && (gal & 3) != 1)
        return fail(HE_EINVAL, "%s: the Galois element %llu is not a power of 5 modulo 4N (conjugate-invariant ring)", who, (unsigned long long)gal);
    uint64_t inv = gal;  // ModInvGaloisElement (:157): the inverse modulo NthRoot, a power of two (five Newton steps double 3 bits to 96)
    for (int i = 0; i < 5; i++) inv *= 2 - gal * inv;
    inv = reduce_gal(inv, Q.logN, Q.type);
    he_handle hix = 0;
    TRY(he_automorphism_index_create(kg.hq, inv, &hix));  // :159
    TmpPoly oq, op;
    int rc = oq.alloc(kg.hq, k->nQk, 1);
    if (rc == HE_OK && k->nPk) rc = op.alloc(kg.hp, k->nPk, 1);
    if (rc == HE_OK) rc = he_automorphism_ntt_with_index(kg.hq, k->nQk - 1, skQ, hix, oq.h);            // :167
    if (rc == HE_OK && k->nPk) rc = he_automorphism_ntt_with_index(kg.hp, k->nPk - 1, skP, hix, op.h);  // :169-171
    if (rc == HE_OK) {
        { Scope sc(&kg.ctx()); }
        rc = keygen_evaluation_key(kg, who, q->d, get<Poly>(oq.h, T_POLY)->d, k->nPk ? get<Poly>(op.h, T_POLY)->d : nullptr, *k, crp.get());  // :173
    }
    (void)he_automorphism_index_destroy(hix);
    return rc;
}
int he_keygen_galois_key(he_handle hk, uint64_t gal_el, he_handle skQ, he_handle skP, he_handle gk) {
    static const char *who = "he_keygen_galois_key";
    GET(kg, KeyGen, hk, T_KEYGEN);
    TRY(rlwe_frame_begin(kg->ctx(), who));
    const int rc = keygen_galois_key(*kg, who, gal_el, skQ, skP, gk);
    const int rs = rlwe_frame_end(kg->ctx());
    return rc != HE_OK ? rc : rs;
}
int he_keygen_galois_keys(he_handle hk, int n, const uint64_t *gal_els, he_handle skQ, he_handle skP, const he_handle *gks) {
    static const char *who = "he_keygen_galois_keys";
    GET(kg, KeyGen, hk, T_KEYGEN);
    TRY(rlwe_frame_begin(kg->ctx(), who));
    if (n < 0 || (n > 0 && (!gal_els || !gks))) return fail(HE_EINVAL, "%s: %d keys with a null array", who, n);
    for (int i = 0; i < n; i++) {  // (every check before the first draw)
        if (!(gal_els[i] & 1) || (kg->ev->be->Q->type == 1 && (gal_els[i] & 3) != 1))
            return fail(HE_EINVAL, "%s: the Galois element %llu is even, or not a power of 5 on a conjugate-invariant ring", who, (unsigned long long)gal_els[i]);
        std::shared_ptr<Evk> k;
        TRY(keygen_evk(*kg, who, gks[i], &k));
        TRY(keygen_sk_for(*kg, who, *k, skQ, skP, "skQ", "skP", nullptr, nullptr));
        for (int j = 0; j < i; j++)
            if (gks[j] == gks[i]) return fail(HE_EINVAL, "%s: gks[%d] and gks[%d] are one key", who, j, i);
    }
    int rc = HE_OK;
    for (int i = 0; i < n && rc == HE_OK; i++) rc = keygen_galois_key(*kg, who, gal_els[i], skQ, skP, gks[i]);  // :189-195, key after key
    const int rs = rlwe_frame_end(kg->ctx());
    return rc != HE_OK ? rc : rs;
}

// ---------------------------------------------------------------------------------------
// multiparty.EvaluationKeyGenProtocol and GaloisKeyGenProtocol (include/hering_multiparty.h; multiparty/keygen_evk.go, keygen_gal.go).
// A share is keygen_evaluation_key with the CRP as its c1; aggregation is one launch over the key storage.
// ---------------------------------------------------------------------------------------
int he_mp_crp_gadget(he_handle hev, he_handle hcrs, he_handle hevk) {
    static const char *who = "he_mp_crp_gadget";
    GET(ev, Evaluator, hev, T_EVAL);
    GET(g, Prng, hcrs, T_PRNG);
    GET(k, Evk, hevk, T_EVK);
    BasisExtender &be = *ev->be;
    Ctx &c = *be.ctx;
    TRY(rlwe_frame_begin(c, who));
    if (k->ev != ev) return fail(HE_EINVAL, "%s: the key belongs to another evaluator", who);
    TRY(evk_shape_for_keygen(*k, who, "the key"));
    { Scope sc(&c); }  // (after the calling thread's queued requests)
    const int N = be.Q->N, nQk = k->nQk, nPk = k->nPk;
    const size_t blk = (size_t)(nQk + nPk) * N;
    const ModConst *const mc[2] = {be.Q->dev.mc, nPk ? be.P->dev.mc : nullptr};
    const int nl[2] = {nQk, nPk};
    const size_t bs[2] = {2 * blk, 2 * blk};
    int rc = HE_OK;
    for (int r = 0; r < k->beta && rc == HE_OK; r++) {  // keygen_evk.go:74-80: us.ReadNew() per (i, j), i outer
        uint64_t *c1 = k->d + ((size_t)2 * r + 1) * blk;
        uint64_t *const out[2] = {c1, c1 + (size_t)nQk * N};
        rc = uniform_read_run(who, c, *g, N, 1, nPk ? 2 : 1, mc, nl, out, bs, false, nullptr);
    }
    const int rs = rlwe_frame_end(c);
    return rc != HE_OK ? rc : rs;
}
int he_mp_evk_gen_share(he_handle hk, he_handle skInQ, he_handle skOutQ, he_handle skOutP, he_handle hcrp, he_handle hshare) {
    static const char *who = "he_mp_evk_gen_share";
    GET(kg, KeyGen, hk, T_KEYGEN);
    TRY(rlwe_frame_begin(kg->ctx(), who));
    std::shared_ptr<Evk> crp, k;
    TRY(keygen_evk(*kg, who, hcrp, &crp));
    TRY(keygen_evk(*kg, who, hshare, &k));
    TRY(evk_same_shape(who, *crp, *k, "crp", "share"));
    std::shared_ptr<Poly> in, oq, op;
    TRY(keygen_poly(*kg, who, skInQ, k->nQk, "skInQ", &in));
    TRY(keygen_sk_for(*kg, who, *k, skOutQ, skOutP, "skOutQ", "skOutP", &oq, &op));
    { Scope sc(&kg->ctx()); }
    return keygen_evaluation_key(*kg, who, in->d, oq->d, op ? op->d : nullptr, *k, crp.get());
}
int he_mp_galois_gen_share(he_handle hk, uint64_t gal_el, he_handle skQ, he_handle skP, he_handle hcrp, he_handle hshare) {
    static const char *who = "he_mp_galois_gen_share";
    GET(kg, KeyGen, hk, T_KEYGEN);
    TRY(rlwe_frame_begin(kg->ctx(), who));
    if (!hcrp) return fail(HE_EHANDLE, "%s: bad Evk handle 0 for crp", who);
    const int rc = keygen_galois_key(*kg, who, gal_el, skQ, skP, hshare, hcrp);
    const int rs = rlwe_frame_end(kg->ctx());
    return rc != HE_OK ? rc : rs;
}
int he_mp_gadget_aggregate(he_handle ha, he_handle hb, int degree, he_handle hout) {
    static const char *who = "he_mp_gadget_aggregate";
    GET(a, Evk, ha, T_EVK);
    GET(b, Evk, hb, T_EVK);
    GET(o, Evk, hout, T_EVK);
    BasisExtender &be = *a->ev->be;
    Ctx &c = *be.ctx;
    TRY(rlwe_frame_begin(c, who));
    if (degree < 0 || degree > 1) return fail(HE_EINVAL, "%s: degree %d is not 0 or 1", who, degree);
    TRY(evk_same_shape(who, *a, *b, "a", "b"));
    TRY(evk_same_shape(who, *a, *o, "a", "out"));
    if (a->nQk + a->nPk > kMaxLimbs) return fail(HE_EINVAL, "%s: %d limbs per row, at most %d", who, a->nQk + a->nPk, kMaxLimbs);
    Scope sc(&c);
    EvkRowsArgs ra;
    evk_rows_args(*a, ra);
    GadgetAggArgs g;
    g.a = a->d; g.b = b->d; g.out = o->d;
    g.blk = ra.blk; g.N = ra.N; g.rows = ra.rows; g.ncomp = degree + 1; g.nl = ra.nq + ra.np; g.mc = ra.mc;
    std::memcpy(g.mod, ra.mod, sizeof g.mod);
    // one Add: words below ma q and mb q give words below (ma + mb - 1) q
    o->word_mul = std::min(Evk::kWordMulCap, std::max<uint64_t>(o->word_mul, a->word_mul + b->word_mul - 1));
    HIP_TRY(launch_gadget_aggregate(g, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    return HE_OK;
}
int he_mp_evk_finalize(he_handle hshare, he_handle hcrp, he_handle hevk) {
    static const char *who = "he_mp_evk_finalize";
    GET(sh, Evk, hshare, T_EVK);
    GET(crp, Evk, hcrp, T_EVK);
    GET(k, Evk, hevk, T_EVK);
    BasisExtender &be = *k->ev->be;
    Ctx &c = *be.ctx;
    TRY(rlwe_frame_begin(c, who));
    TRY(evk_same_shape(who, *sh, *k, "share", "evk"));
    TRY(evk_same_shape(who, *crp, *k, "crp", "evk"));
    Scope sc(&c);
    const size_t blk = (size_t)(k->nQk + k->nPk) * be.Q->N;
    // evk.Value[i][j][0].Copy(m[i][j][0]); evk.Value[i][j][1].Copy(p[i][j]) (keygen_evk.go:233-238): the components lie 2 blk apart
    if (sh != k) HIP_TRY(hipMemcpy2DAsync(k->d, 2 * blk * 8, sh->d, 2 * blk * 8, blk * 8, (size_t)k->beta, hipMemcpyDeviceToDevice, c.stream));
    if (crp != k) HIP_TRY(hipMemcpy2DAsync(k->d + blk, 2 * blk * 8, crp->d + blk, 2 * blk * 8, blk * 8, (size_t)k->beta, hipMemcpyDeviceToDevice, c.stream));
    k->word_mul = std::min(Evk::kWordMulCap, std::max(sh->word_mul, crp->word_mul));
    TRY(evk_derive(*k));
    HIP_TRY(hipStreamSynchronize(c.stream));
    return HE_OK;
}

// RelinearizationKeyGenProtocol (multiparty/keygen_relin.go).  A round draws row by row into a staging buffer of small values and then
// makes, once for the whole share: the expansion into the Q and P limbs of every row (and component), ONE transform, ONE launch of
// the round's kernel.  round 1: crp holds the CRP, u = the ephemeral key just drawn, 2 Gaussians per row (component 0's, then
// component 1's) in the order j outer, i inner; round 2: `in` is the aggregated round-one share, 1 Gaussian per row, i outer.
static int rkg_round(KeyGen &kg, const char *who, int round, const Evk &in, Evk &k, const uint64_t *skQ, const uint64_t *skP, const uint64_t *uQ,
                     const uint64_t *uP) {
    BasisExtender &be = *kg.ev->be;
    Ctx &c = *be.ctx;
    Prng &g = *kg.prng_keep;
    const int N = be.Q->N, R = k.beta, nQk = k.nQk, nPk = k.nPk, per = round == 1 ? 2 : 1;
    const size_t blk = (size_t)(nQk + nPk) * N;
    const size_t stage_bytes = (size_t)R * per * N * 8;  // the small values, [R][per][N]: outside the arena, which every draw resets
    uint64_t *d_e = nullptr;
    {
        Scope sc(&c);
        HIP_TRY(c.pool_take(stage_bytes, (void **)&d_e));
    }
    std::vector<int> order;
    if (round == 1 && k.pw2) {  // (:133-136)
        const int nmax = *std::max_element(k.nj.begin(), k.nj.end());
        for (int j = 0; j < nmax; j++)
            for (size_t i = 0; i < k.nj.size(); i++)
                if (j < k.nj[i]) order.push_back(k.prefix[i] + j);
    } else {
        for (int r = 0; r < R; r++) order.push_back(r);
    }
    int rc = HE_OK;
    for (size_t t = 0; t < order.size() && rc == HE_OK; t++) {
        const int r = order[t];
        rc = gaussian_parse_run(who, c, g, N, per, kg.sigma, kg.bound, [&](const uint64_t *vals) -> int {
            HIP_TRY(hipMemcpyAsync(d_e + (size_t)r * per * N, vals, (size_t)per * N * 8, hipMemcpyDeviceToDevice, c.stream));
            return HE_OK;
        });
    }
    Scope sc(&c);
    std::vector<uint64_t> G;
    if (rc == HE_OK) rc = [&]() -> int {
        TRY(c.arena_reserve((size_t)R * nQk + 8));
        // component 0 of every row (round 2) or both components (round 1): entries blk (2 blk) words apart
        const size_t bs = round == 1 ? blk : 2 * blk;
        const int B = R * per;
        const View v{k.d, bs};
        HIP_TRY(launch_sampler_expand(be.qp.mc, d_e, true, false, false, nullptr, nullptr, v, N, nQk, B, c.stream));
        if (nPk)
            HIP_TRY(launch_sampler_expand(be.qp.mc + be.LQ, d_e, true, false, false, nullptr, nullptr, View{k.d + (size_t)nQk * N, bs}, N, nPk, B, c.stream));
        LimbTab tab = ident_tab(nQk + nPk);
        for (int i = 0; i < nPk; i++) tab.mod[nQk + i] = (uint8_t)(be.LQ + i);
        HIP_TRY(be_ntt(be, tab, v, v, B, false, NTT_REDUCE_INPUT));  // ringQP.NTT (:144, :176, :226)
        EvkRowsArgs ra;
        evk_rows_args(k, ra);
        RkgRowsArgs a;
        a.share = k.d; a.in = in.d; a.blk = blk; a.N = N; a.rows = R; a.nq = nQk; a.np = nPk; a.mc = ra.mc;
        std::memcpy(a.mod, ra.mod, sizeof a.mod);
        a.skQ = skQ; a.skP = skP; a.uQ = uQ; a.uP = uP;
        if (round == 1) TRY(gadget_table_upload(c, k, G, &a.G, false));
        c.acct((round == 1 ? 5.0 : 4.0) * (nQk + nPk), 0, R, N);
        HIP_TRY(round == 1 ? launch_rkg_round_one(a, c.stream) : launch_rkg_round_two(a, c.stream));
        k.word_mul = round == 1 ? 1 : 2;  // (round two leaves words in [0, 2q))
        return HE_OK;
    }();
    (void)hipMemsetAsync(d_e, 0, stage_bytes, c.stream);
    HIP_TRY(hipStreamSynchronize(c.stream));
    c.pool_give(stage_bytes, d_e);
    return rc;
}
// the operands two rounds share: the two keys of one shape and distinct, sk and the ephemeral key at the share's levels
static int rkg_operands(KeyGen &kg, const char *who, he_handle hin, he_handle hshare, const char *nin, he_handle skQ, he_handle skP, he_handle ephQ,
                        he_handle ephP, std::shared_ptr<Evk> *in, std::shared_ptr<Evk> *k, std::shared_ptr<Poly> pol[4]) {
    TRY(keygen_evk(kg, who, hin, in));
    TRY(keygen_evk(kg, who, hshare, k));
    TRY(evk_same_shape(who, **in, **k, nin, "the share"));
    if (*in == *k) return fail(HE_EINVAL, "%s: %s and the share are one key", who, nin);
    TRY(keygen_sk_for(kg, who, **k, skQ, skP, "skQ", "skP", &pol[0], &pol[1]));
    TRY(keygen_sk_for(kg, who, **k, ephQ, ephP, "ephQ", "ephP", &pol[2], &pol[3]));
    return HE_OK;
}
int he_mp_rkg_round_one(he_handle hk, he_handle skQ, he_handle skP, he_handle hcrp, he_handle ephQ, he_handle ephP, he_handle hshare) {
    static const char *who = "he_mp_rkg_round_one";
    GET(kg, KeyGen, hk, T_KEYGEN);
    TRY(rlwe_frame_begin(kg->ctx(), who));
    std::shared_ptr<Evk> crp, k;
    std::shared_ptr<Poly> pol[4];
    TRY(rkg_operands(*kg, who, hcrp, hshare, "crp", skQ, skP, ephQ, ephP, &crp, &k, pol));
    const he_handle outs[2] = {ephQ, k->nPk ? ephP : 0}, others[2] = {skQ, k->nPk ? skP : 0};
    TRY(rlwe_distinct(who, outs, 2, others, 2));
    // u (:116-121): the ternary Read at the level of the ephemeral key's own limbs (the reference's sampler stands at the parameters'
    // top level), then the extension, NTT and MForm at the share's levels
    const int levelU = std::min(pol[2]->nlimbs, kg->maxQ() + 1) - 1;
    int rc = he_sampler_ternary_read(kg->hq, levelU, kg->prng, kg->xs_p, 0, 0, ephQ);
    if (rc == HE_OK) rc = keygen_sk_finish(*kg, k->nQk - 1, k->nPk - 1, ephQ, ephP);
    if (rc == HE_OK) {
        { Scope sc(&kg->ctx()); }
        rc = rkg_round(*kg, who, 1, *crp, *k, pol[0]->d, pol[1] ? pol[1]->d : nullptr, pol[2]->d, pol[3] ? pol[3]->d : nullptr);
    }
    const int rs = rlwe_frame_end(kg->ctx());
    return rc != HE_OK ? rc : rs;
}
int he_mp_rkg_round_two(he_handle hk, he_handle ephQ, he_handle ephP, he_handle skQ, he_handle skP, he_handle hround1, he_handle hshare) {
    static const char *who = "he_mp_rkg_round_two";
    GET(kg, KeyGen, hk, T_KEYGEN);
    TRY(rlwe_frame_begin(kg->ctx(), who));
    std::shared_ptr<Evk> r1, k;
    std::shared_ptr<Poly> pol[4];
    TRY(rkg_operands(*kg, who, hround1, hshare, "round1", skQ, skP, ephQ, ephP, &r1, &k, pol));
    if (r1->word_mul != 1) return fail(HE_EINVAL, "%s: round1 holds lazy words; an aggregated round-one share is canonical", who);
    { Scope sc(&kg->ctx()); }
    return rkg_round(*kg, who, 2, *r1, *k, pol[0]->d, pol[1] ? pol[1]->d : nullptr, pol[2]->d, pol[3] ? pol[3]->d : nullptr);
}
int he_mp_rlk_finalize(he_handle hround1, he_handle hround2, he_handle hrlk) {
    static const char *who = "he_mp_rlk_finalize";
    GET(r1, Evk, hround1, T_EVK);
    GET(r2, Evk, hround2, T_EVK);
    GET(k, Evk, hrlk, T_EVK);
    BasisExtender &be = *k->ev->be;
    Ctx &c = *be.ctx;
    TRY(rlwe_frame_begin(c, who));
    TRY(evk_same_shape(who, *r1, *k, "round1", "rlk"));
    TRY(evk_same_shape(who, *r2, *k, "round2", "rlk"));
    if (k->nQk + k->nPk > kMaxLimbs) return fail(HE_EINVAL, "%s: %d limbs per row, at most %d", who, k->nQk + k->nPk, kMaxLimbs);
    Scope sc(&c);
    EvkRowsArgs ra;
    evk_rows_args(*k, ra);
    GadgetAggArgs g;
    g.a = r2->d; g.b = r1->d; g.out = k->d;
    g.blk = ra.blk; g.N = ra.N; g.rows = ra.rows; g.ncomp = 2; g.nl = ra.nq + ra.np; g.mc = ra.mc;
    std::memcpy(g.mod, ra.mod, sizeof g.mod);
    HIP_TRY(launch_rlk_finalize(g, c.stream));  // the two MForms (:272-273)
    k->word_mul = 1;
    TRY(evk_derive(*k));
    HIP_TRY(hipStreamSynchronize(c.stream));
    return HE_OK;
}

// PublicKeyGenProtocol.GenShare (multiparty/keygen_cpk.go:62-75) and KeySwitchProtocol.GenShare (keyswitch_sk.go:82-118): polynomial-sized,
// compositions of the ring and sampler entries.
int he_mp_pk_gen_share(he_handle hk, he_handle skQ, he_handle skP, he_handle crpQ, he_handle crpP, he_handle shareQ, he_handle shareP) {
    static const char *who = "he_mp_pk_gen_share";
    GET(kg, KeyGen, hk, T_KEYGEN);
    TRY(rlwe_frame_begin(kg->ctx(), who));
    const int levelQ = kg->maxQ(), levelP = kg->maxP();  // params.RingQP(): the top levels
    const he_handle hs[6] = {skQ, crpQ, shareQ, skP, crpP, shareP};
    const char *const names[6] = {"skQ", "crpQ", "shareQ", "skP", "crpP", "shareP"};
    for (int i = 0; i < (levelP >= 0 ? 6 : 3); i++) TRY(keygen_poly(*kg, who, hs[i], (i < 3 ? levelQ : levelP) + 1, names[i], nullptr));
    const he_handle outs[2] = {shareQ, levelP >= 0 ? shareP : 0}, others[4] = {skQ, crpQ, levelP >= 0 ? skP : 0, levelP >= 0 ? crpP : 0};
    TRY(rlwe_distinct(who, outs, 2, others, 4));
    int rc = he_sampler_gaussian_read(kg->hq, levelQ, kg->prng, kg->sigma, kg->bound, 0, 0, shareQ);  // :65
    if (rc == HE_OK && levelP >= 0) rc = he_centered_lift(kg->hev, 3, shareQ, levelQ + 1, levelQ, shareQ, levelP, shareP);  // :67-69
    if (rc == HE_OK) rc = he_ntt(kg->hq, levelQ, shareQ, shareQ);  // :71
    if (rc == HE_OK && levelP >= 0) rc = he_ntt(kg->hp, levelP, shareP, shareP);
    if (rc == HE_OK) rc = he_mform(kg->hq, levelQ, shareQ, shareQ);  // :72
    if (rc == HE_OK && levelP >= 0) rc = he_mform(kg->hp, levelP, shareP, shareP);
    if (rc == HE_OK) rc = he_binop(kg->hq, levelQ, HE_MUL_COEFFS_MONTGOMERY_THEN_SUB, skQ, crpQ, shareQ);  // :74
    if (rc == HE_OK && levelP >= 0) rc = he_binop(kg->hp, levelP, HE_MUL_COEFFS_MONTGOMERY_THEN_SUB, skP, crpP, shareP);
    const int rs = rlwe_frame_end(kg->ctx());
    return rc != HE_OK ? rc : rs;
}
int he_mp_cks_gen_share(he_handle hk, int level, he_handle skInQ, he_handle skOutQ, he_handle c1, int is_ntt, double sigma, double bound,
                        he_handle share) {
    static const char *who = "he_mp_cks_gen_share";
    GET(kg, KeyGen, hk, T_KEYGEN);
    TRY(rlwe_frame_begin(kg->ctx(), who));
    if (level < 0 || level > kg->maxQ()) return fail(HE_EINVAL, "%s: level %d, the ring has levels 0..%d", who, level, kg->maxQ());
    if (!(sigma > 0.0) || sigma > 0x1p53 || !(bound >= 0.0) || bound > 0x1p62)
        return fail(HE_EINVAL, "%s: noise = {%g, %g}: sigma in (0, 2^53] and bound in [0, 2^62] (hering_sampler.h)", who, sigma, bound);
    const he_handle ins[3] = {skInQ, skOutQ, c1};
    const char *const names[3] = {"skInQ", "skOutQ", "c1"};
    for (int i = 0; i < 3; i++) TRY(keygen_poly(*kg, who, ins[i], level + 1, names[i], nullptr));
    TRY(keygen_poly(*kg, who, share, level + 1, "share", nullptr));
    TRY(rlwe_distinct(who, &share, 1, ins, 3));
    TmpPoly delta, buf;  // sk_in - sk_out and the Gaussian: cleared before they go back to the pool
    TRY(delta.alloc(kg->hq, level + 1, 1));
    TRY(buf.alloc(kg->hq, level + 1, 1));
    int rc = he_sub(kg->hq, level, skInQ, skOutQ, delta.h);  // :92
    if (rc == HE_OK && !is_ntt) rc = he_ntt_lazy(kg->hq, level, c1, buf.h);  // :95-97
    if (rc == HE_OK) rc = he_mul_coeffs_montgomery_lazy(kg->hq, level, is_ntt ? c1 : buf.h, delta.h, share);  // :103
    if (rc == HE_OK && !is_ntt) {  // :105-108
        rc = he_intt_lazy(kg->hq, level, share, share);
        if (rc == HE_OK) rc = he_sampler_gaussian_read(kg->hq, level, kg->prng, sigma, bound, 0, 1, share);
    } else if (rc == HE_OK) {      // :110-114
        rc = he_sampler_gaussian_read(kg->hq, level, kg->prng, sigma, bound, 0, 0, buf.h);
        if (rc == HE_OK) rc = he_ntt(kg->hq, level, buf.h, buf.h);
        if (rc == HE_OK) rc = he_add(kg->hq, level, share, buf.h, share);
    }
    const int rs = rlwe_frame_end(kg->ctx());
    return rc != HE_OK ? rc : rs;
}
// PublicKeySwitchProtocol.GenShare (multiparty/keyswitch_pk.go:69-105): EncryptZero under the encryptor's public key, from the
// encryptor's own source, then the c1 s term and a Gaussian from the protocol's noise source.
int he_mp_pcks_gen_share(he_handle henc, he_handle hnoise, int level, he_handle skQ, he_handle c1, int is_ntt, int is_montgomery, double sigma,
                         double bound, he_handle share0, he_handle share1) {
    static const char *who = "he_mp_pcks_gen_share";
    GET(enc, Encryptor, henc, T_ENCRYPTOR);
    GET(g, Prng, hnoise, T_PRNG);
    TRY(rlwe_frame_begin(enc->ctx(), who));
    if (level < 0 || level > enc->maxQ()) return fail(HE_EINVAL, "%s: level %d, the ring has levels 0..%d", who, level, enc->maxQ());
    if (!(sigma > 0.0) || sigma > 0x1p53 || !(bound >= 0.0) || bound > 0x1p62)
        return fail(HE_EINVAL, "%s: noise = {%g, %g}: sigma in (0, 2^53] and bound in [0, 2^62] (hering_sampler.h)", who, sigma, bound);
    {
        std::lock_guard<std::mutex> lk(enc->mu);
        if (enc->kind != 2) return fail(HE_EINVAL, "%s: the encryptor is not bound to a public key (he_encryptor_set_key, kind 2)", who);
    }
    const he_handle hs[4] = {skQ, c1, share0, share1};
    const char *const names[4] = {"skQ", "c1", "share0", "share1"};
    for (int i = 0; i < 4; i++) {  // (a share above the ciphertext's level: HE_EINVAL, where the reference encrypts at one level and adds at another)
        auto p = get<Poly>(hs[i], T_POLY);
        if (!p) return fail(HE_EHANDLE, "%s: bad Poly handle for %s", who, names[i]);
        if (p->ctx.get() != &enc->ctx() || p->N != enc->ev->be->Q->N || p->batch != 1 || p->nlimbs < level + 1)
            return fail(HE_EINVAL, "%s: %s must be one polynomial of the encryptor's ringQ with %d limbs", who, names[i], level + 1);
    }
    const he_handle outs[2] = {share0, share1}, ins[2] = {skQ, c1};
    TRY(rlwe_distinct(who, outs, 2, ins, 2));
    TmpPoly buf;  // c1 s and the noise: cleared before it goes back to the pool
    TRY(buf.alloc(enc->hq, level + 1, 1));
    int rc = he_encrypt_zero(henc, level, is_ntt, is_montgomery, share0, share1);  // :77-88
    if (rc == HE_OK && is_ntt) {  // :93-97
        rc = he_mul_coeffs_montgomery_then_add(enc->hq, level, c1, skQ, share0);
        if (rc == HE_OK) rc = he_sampler_gaussian_read(enc->hq, level, hnoise, sigma, bound, 0, 0, buf.h);
        if (rc == HE_OK) rc = he_ntt(enc->hq, level, buf.h, buf.h);
    } else if (rc == HE_OK) {     // :98-103
        rc = he_ntt_lazy(enc->hq, level, c1, buf.h);
        if (rc == HE_OK) rc = he_mul_coeffs_montgomery_lazy(enc->hq, level, buf.h, skQ, buf.h);
        if (rc == HE_OK) rc = he_intt(enc->hq, level, buf.h, buf.h);
        if (rc == HE_OK) rc = he_sampler_gaussian_read(enc->hq, level, hnoise, sigma, bound, 0, 1, buf.h);
    }
    if (rc == HE_OK) rc = he_add(enc->hq, level, share0, buf.h, share0);
    const int rs = rlwe_frame_end(enc->ctx());
    return rc != HE_OK ? rc : rs;
}

// ---------------------------------------------------------------------------------------
// rgsw.Encryptor and blindrot.GenEvaluationKeyNew (include/hering_rgsw_encryptor.h; core/rgsw/encryptor.go, blindrot/keys.go).  A table
// of RGSW ciphertexts draws row by row into the keys' own storage, as keygen_evaluation_key does, and finishes every row of a
// chunk of ciphertexts at once (launch_rgsw_table_finish).
// ---------------------------------------------------------------------------------------
// the staging of a chunk: N words of small values and one (nQk + nPk)-limb slab entry per table row
static constexpr size_t kRgswStageBudget = (size_t)256 << 20;
static int rgsw_chunk_keys(int n, int R, size_t blk, int N) {
    const int cap = 65535 / (2 * R);  // table rows are a grid coordinate and a batch (launch_rgsw_table_finish, be_ntt)
    size_t chunk = kRgswStageBudget / ((size_t)2 * R * (blk + N) * 8);
    const char *s = getenv("HERING_RGSW_CHUNK_KEYS");  // (set-up code: read at each call)
    if (s && atoi(s) > 0) chunk = (size_t)atoi(s);
    return (int)std::max<size_t>(1, std::min<size_t>({chunk, (size_t)cap, (size_t)n}));
}
// the operands every entry shares: the bound secret key and the 2 n keys, keys[2 k + u] = gadget ciphertext u of ciphertext k
struct RgswOperands {
    std::shared_ptr<Poly> skQ, skP;
    he_handle hskQ = 0, hskP = 0;
    std::vector<std::shared_ptr<Evk>> keys;
};
static int rgsw_operands(Encryptor &e, const char *who, int n, const he_handle *h0, const he_handle *h1, RgswOperands &o) {
    if (n < 1 || !h0 || !h1) return fail(HE_EINVAL, "%s: %d ciphertexts with a null array", who, n);
    int kind;
    {
        std::lock_guard<std::mutex> lk(e.mu);
        kind = e.kind;
        o.hskQ = e.key[0];
        o.hskP = e.key[1];
    }
    if (kind != 1) return fail(HE_EINVAL, "%s: %s; only secret-key encryption is supported", who, kind ? "a public key is bound" : "the encryptor has no encryption key");
    o.keys.resize((size_t)2 * n);
    for (int k = 0; k < n; k++)
        for (int u = 0; u < 2; u++) {
            auto key = get<Evk>(u ? h1[k] : h0[k], T_EVK);
            if (!key) return fail(HE_EHANDLE, "%s: bad Evk handle for rgsw%d[%d]", who, u, k);
            if (key->ev != e.ev) return fail(HE_EINVAL, "%s: rgsw%d[%d] belongs to another evaluator than the encryptor", who, u, k);
            const Evk &f = k || u ? *o.keys[0] : *key;
            if (key->beta != f.beta || key->nQk != f.nQk || key->nPk != f.nPk || key->pw2 != f.pw2 || key->nj != f.nj)
                return fail(HE_EINVAL, "%s: rgsw%d[%d] differs in shape from rgsw0[0]", who, u, k);
            o.keys[(size_t)2 * k + u] = key;
        }
    const Evk &f = *o.keys[0];
    TRY(evk_shape_for_keygen(f, who, "the ciphertext"));
    if (2 * f.beta > 65535) return fail(HE_EINVAL, "%s: %d rows per gadget ciphertext", who, f.beta);
    {
        std::vector<const Evk *> seen;
        for (const auto &k : o.keys) seen.push_back(k.get());
        std::sort(seen.begin(), seen.end());
        if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return fail(HE_EINVAL, "%s: two of the output keys are one key", who);
    }
    const int N = e.ev->be->Q->N;
    auto sk_part = [&](he_handle h, int limbs, const char *name, std::shared_ptr<Poly> *out) -> int {
        auto p = get<Poly>(h, T_POLY);
        if (!p) return fail(HE_EHANDLE, "%s: bad Poly handle for %s of the bound key", who, name);
        if (p->ctx.get() != &e.ctx() || p->N != N || p->nlimbs < limbs || p->batch != 1)
            return fail(HE_EINVAL, "%s: %s of the bound key must be one polynomial of the encryptor's rings with %d limbs", who, name, limbs);
        *out = p;
        return HE_OK;
    };
    TRY(sk_part(o.hskQ, f.nQk, "sk.Q", &o.skQ));
    if (f.nPk) {
        if (!o.hskP) return fail(HE_EINVAL, "%s: the key was bound without its P part, which this call reads", who);
        TRY(sk_part(o.hskP, f.nPk, "sk.P", &o.skP));
    }
    return HE_OK;
}
// n successive rgsw.Encryptor.Encrypt calls without the frame.  pts: device words of the plaintexts (entry s at pts + s pt_stride,
// nQk limbs, NTT and Montgomery; null: every sel is -1); sel: host, checked by the caller.
static int rgsw_encrypt_table(Encryptor &e, const char *who, const RgswOperands &o, const uint64_t *pts, size_t pt_stride, const int32_t *sel, int n) {
    BasisExtender &be = *e.ev->be;
    Ctx &c = *be.ctx;
    Prng &g = *e.prng_keep;
    const Evk &f = *o.keys[0];
    const int N = be.Q->N, R = f.beta, nQk = f.nQk, nPk = f.nPk;
    const size_t blk = (size_t)(nQk + nPk) * N;
    const int chunk = rgsw_chunk_keys(n, R, blk, N);
    // the small values of every row's Gaussian, [table rows][N], and the slab that becomes NTT(e), [table rows][nQk + nPk][N]: outside
    // the arena, which every draw resets
    const size_t e_bytes = (size_t)chunk * 2 * R * N * 8, slab_bytes = (size_t)chunk * 2 * R * blk * 8;
    uint64_t *d_e = nullptr, *slab = nullptr;
    {
        Scope sc(&c);
        HIP_TRY(c.pool_take(e_bytes, (void **)&d_e));
        HIP_TRY(c.pool_take(slab_bytes, (void **)&slab));
    }
    int rc = HE_OK;
    const ModConst *const mc[2] = {be.Q->dev.mc, nPk ? be.P->dev.mc : nullptr};
    const int nl[2] = {nQk, nPk};
    const size_t bs[2] = {2 * blk, 2 * blk};
    const std::vector<uint64_t> G = gadget_table(f);
    std::vector<uint64_t> bases;
    for (int kb = 0; kb < n && rc == HE_OK; kb += chunk) {
        const int nk = std::min(chunk, n - kb), T = nk * 2 * R;
        // encryptor.go:92-118: per ciphertext, per row (i, j), one encryptZeroSk on Value[0][i][j] and one on Value[1][i][j]
        for (int k = 0; k < nk && rc == HE_OK; k++)
            for (int r = 0; r < R && rc == HE_OK; r++)
                for (int u = 0; u < 2 && rc == HE_OK; u++) {
                    uint64_t *c1 = o.keys[(size_t)2 * (kb + k) + u]->d + ((size_t)2 * r + 1) * blk;
                    uint64_t *const out[2] = {c1, c1 + (size_t)nQk * N};
                    rc = uniform_read_run(who, c, g, N, 1, nPk ? 2 : 1, mc, nl, out, bs, false, nullptr);
                    if (rc != HE_OK) break;
                    uint64_t *dst = d_e + ((size_t)(k * 2 + u) * R + r) * N;
                    rc = gaussian_parse_run(who, c, g, N, 1, e.sigma, e.bound, [&](const uint64_t *vals) -> int {
                        HIP_TRY(hipMemcpyAsync(dst, vals, (size_t)N * 8, hipMemcpyDeviceToDevice, c.stream));
                        return HE_OK;
                    });
                }
        if (rc != HE_OK) break;
        Scope sc(&c);
        rc = [&]() -> int {
            const size_t sel_words = ((size_t)nk + 1) / 2;
            TRY(c.arena_reserve(G.size() + (size_t)2 * nk + sel_words + 16));
            const View sv{slab, blk};
            // encryptor.go:411-414 for every table row at once: the Gaussian words on the Q limbs and their centred copies on the P limbs
            HIP_TRY(launch_sampler_expand(be.qp.mc, d_e, true, false, false, nullptr, nullptr, sv, N, nQk, T, c.stream));
            if (nPk)
                HIP_TRY(launch_sampler_expand(be.qp.mc + be.LQ, d_e, true, false, false, nullptr, nullptr, View{slab + (size_t)nQk * N, blk}, N, nPk, T, c.stream));
            LimbTab tab = ident_tab(nQk + nPk);
            for (int i = 0; i < nPk; i++) tab.mod[nQk + i] = (uint8_t)(be.LQ + i);
            HIP_TRY(be_ntt(be, tab, sv, sv, T, false, NTT_REDUCE_INPUT));  // :416-418
            RgswTableArgs a;
            a.e = slab; a.blk = blk; a.N = N; a.rows = R; a.nkeys = nk; a.nq = nQk; a.np = nPk;
            a.mc = be.qp.mc;
            for (int i = 0; i < nQk; i++) a.mod[i] = (uint8_t)i;
            for (int i = 0; i < nPk; i++) a.mod[nQk + i] = (uint8_t)(be.LQ + i);
            a.skQ = o.skQ->d; a.skP = nPk ? o.skP->d : nullptr;
            bases.resize((size_t)2 * nk);
            for (int i = 0; i < 2 * nk; i++) bases[(size_t)i] = (uint64_t)(uintptr_t)o.keys[(size_t)2 * kb + i]->d;
            uint64_t *d_bases = c.arena_take(bases.size());
            HIP_TRY(hipMemcpyAsync(d_bases, bases.data(), bases.size() * 8, hipMemcpyHostToDevice, c.stream));
            a.keys = reinterpret_cast<uint64_t *const *>(d_bases);
            uint64_t *d_sel = nullptr;
            if (pts) {
                uint64_t *d_G = c.arena_take(G.size());
                HIP_TRY(hipMemcpyAsync(d_G, G.data(), G.size() * 8, hipMemcpyHostToDevice, c.stream));
                d_sel = c.arena_take(sel_words);
                HIP_TRY(hipMemcpyAsync(d_sel, sel + kb, (size_t)nk * 4, hipMemcpyHostToDevice, c.stream));
                a.pts = pts; a.pt_stride = pt_stride; a.G = d_G; a.sel = reinterpret_cast<const int32_t *>(d_sel);
            }
            c.acct(3.0 * (nQk + nPk), 0, T, N);
            HIP_TRY(launch_rgsw_table_finish(a, c.stream));  // :420-425 and AddPolyTimesGadgetVectorToGadgetCiphertext with two keys
            if (d_sel) HIP_TRY(hipMemsetAsync(d_sel, 0, sel_words * 8, c.stream));
            for (int i = 0; i < 2 * nk; i++) {
                Evk &k = *o.keys[(size_t)2 * kb + i];
                TRY(evk_derive(k));
                k.word_mul = 1;
            }
            HIP_TRY(hipStreamSynchronize(c.stream));  // (bases and sel are host memory of this call)
            return HE_OK;
        }();
    }
    Scope sc(&c);
    (void)hipMemsetAsync(d_e, 0, e_bytes, c.stream);
    (void)hipMemsetAsync(slab, 0, slab_bytes, c.stream);
    HIP_TRY(hipStreamSynchronize(c.stream));
    c.pool_give(e_bytes, d_e);
    c.pool_give(slab_bytes, slab);
    return rc;
}
// the plaintexts of a table: one polynomial of the encryptor's ringQ with at least `limbs` limbs
static int rgsw_plaintexts(const Encryptor &e, const char *who, he_handle h, int limbs, std::shared_ptr<Poly> *out) {
    auto p = get<Poly>(h, T_POLY);
    if (!p) return fail(HE_EHANDLE, "%s: bad Poly handle for the plaintext", who);
    if (p->ctx.get() != &e.ctx() || p->N != e.ev->be->Q->N || p->nlimbs < limbs)
        return fail(HE_EINVAL, "%s: the plaintext must be a polynomial of the encryptor's ringQ with %d limbs", who, limbs);
    *out = p;
    return HE_OK;
}
static int rgsw_check_sel(const char *who, const int32_t *sel, int n, int m) {
    if (!sel) return fail(HE_EINVAL, "%s: null selection", who);
    for (int k = 0; k < n; k++)
        if (sel[k] < -1 || sel[k] >= m) return fail(HE_EINVAL, "%s: sel[%d] = %d is not in [-1, %d)", who, k, (int)sel[k], m);
    return HE_OK;
}
int he_rgsw_encrypt_table(he_handle henc, he_handle hpts, const int32_t *sel, int n, const he_handle *rgsw0, const he_handle *rgsw1) {
    static const char *who = "he_rgsw_encrypt_table";
    GET(e, Encryptor, henc, T_ENCRYPTOR);
    TRY(rlwe_frame_begin(e->ctx(), who));
    RgswOperands o;
    TRY(rgsw_operands(*e, who, n, rgsw0, rgsw1, o));
    std::shared_ptr<Poly> pts;
    if (hpts) TRY(rgsw_plaintexts(*e, who, hpts, o.keys[0]->nQk, &pts));
    TRY(rgsw_check_sel(who, sel, n, pts ? pts->batch : 0));
    { Scope sc(&e->ctx()); }  // (after the calling thread's queued requests)
    const int rc = rgsw_encrypt_table(*e, who, o, pts ? pts->d : nullptr, pts ? pts->view().bstride : 0, sel, n);
    const int rs = rlwe_frame_end(e->ctx());
    return rc != HE_OK ? rc : rs;
}
int he_rgsw_encrypt(he_handle henc, he_handle hpt, int pt_is_ntt, int pt_is_montgomery, he_handle rgsw0, he_handle rgsw1) {
    static const char *who = "he_rgsw_encrypt";
    GET(e, Encryptor, henc, T_ENCRYPTOR);
    TRY(rlwe_frame_begin(e->ctx(), who));
    RgswOperands o;
    TRY(rgsw_operands(*e, who, 1, &rgsw0, &rgsw1, o));
    const int levelQ = o.keys[0]->nQk - 1;
    std::shared_ptr<Poly> pt;
    TmpPoly buf;  // buffQP.Q (:44)
    if (hpt) {
        TRY(rgsw_plaintexts(*e, who, hpt, levelQ + 1, &pt));
        if (pt->batch != 1) return fail(HE_EINVAL, "%s: the plaintext has %d entries; one polynomial is expected", who, pt->batch);
        if (!pt_is_ntt || !pt_is_montgomery) {  // :47-60
            TRY(buf.alloc(e->hq, levelQ + 1, 1));
            he_handle src = hpt;
            if (!pt_is_ntt) {
                TRY(he_ntt(e->hq, levelQ, src, buf.h));
                src = buf.h;
            }
            if (!pt_is_montgomery) TRY(he_mform(e->hq, levelQ, src, buf.h));
            pt = get<Poly>(buf.h, T_POLY);
        }
    }
    { Scope sc(&e->ctx()); }
    const int32_t sel = pt ? 0 : -1;
    const int rc = rgsw_encrypt_table(*e, who, o, pt ? pt->d : nullptr, pt ? pt->view().bstride : 0, &sel, 1);
    const int rs = rlwe_frame_end(e->ctx());
    return rc != HE_OK ? rc : rs;
}
int he_rgsw_encrypt_zero(he_handle henc, he_handle rgsw0, he_handle rgsw1) {
    static const char *who = "he_rgsw_encrypt_zero";
    GET(e, Encryptor, henc, T_ENCRYPTOR);
    TRY(rlwe_frame_begin(e->ctx(), who));
    RgswOperands o;
    TRY(rgsw_operands(*e, who, 1, &rgsw0, &rgsw1, o));
    { Scope sc(&e->ctx()); }
    const int32_t sel = -1;
    const int rc = rgsw_encrypt_table(*e, who, o, nullptr, 0, &sel, 1);
    const int rs = rlwe_frame_end(e->ctx());
    return rc != HE_OK ? rc : rs;
}
// blindrot.GenEvaluationKeyNew (keys.go:46-108)
int he_blindrot_gen_evaluation_key(he_handle henc, he_handle hkgen, he_handle hringLWE, he_handle hskLWE, int n, const he_handle *rgsw0,
                                   const he_handle *rgsw1, const he_handle *gks) {
    static const char *who = "he_blindrot_gen_evaluation_key";
    constexpr int kWindowSize = 10;  // keys.go:14
    GET(e, Encryptor, henc, T_ENCRYPTOR);
    GET(kg, KeyGen, hkgen, T_KEYGEN);
    GET(rl, Ring, hringLWE, T_RING);
    TRY(rlwe_frame_begin(e->ctx(), who));
    if (kg->ev != e->ev) return fail(HE_EINVAL, "%s: the generator belongs to another evaluator than the encryptor", who);
    const Ring &Q = *e->ev->be->Q;
    if (Q.type != 0) return fail(HE_EINVAL, "%s: a blind rotation runs on a standard ring", who);
    if (rl->ctx.get() != &e->ctx()) return fail(HE_EINVAL, "%s: ringLWE belongs to another context", who);
    if (n != rl->N) return fail(HE_EINVAL, "%s: %d ciphertexts for an LWE ring of degree %d", who, n, rl->N);
    auto skl = get<Poly>(hskLWE, T_POLY);
    if (!skl) return fail(HE_EHANDLE, "%s: bad Poly handle for skLWE", who);
    if (skl->ctx != rl->ctx || skl->N != rl->N || skl->batch != 1) return fail(HE_EINVAL, "%s: skLWE must be one polynomial of ringLWE", who);
    RgswOperands o;
    TRY(rgsw_operands(*e, who, n, rgsw0, rgsw1, o));
    if (!gks) return fail(HE_EINVAL, "%s: null array of Galois keys", who);
    uint64_t gal_els[kWindowSize + 1];  // :94-99
    const uint64_t mask = (uint64_t)2 * Q.N - 1;
    uint64_t pw = 1;
    for (int i = 0; i < kWindowSize; i++) gal_els[i] = pw = pw * 5 & mask;
    gal_els[kWindowSize] = (uint64_t)2 * Q.N - 5;
    for (int i = 0; i <= kWindowSize; i++) {  // (every check before the first draw)
        std::shared_ptr<Evk> k;
        TRY(keygen_evk(*kg, who, gks[i], &k));
        TRY(keygen_sk_for(*kg, who, *k, o.hskQ, o.hskP, "sk.Q", "sk.P", nullptr, nullptr));
        for (int j = 0; j < i; j++)
            if (gks[j] == gks[i]) return fail(HE_EINVAL, "%s: gks[%d] and gks[%d] are one key", who, j, i);
        for (const auto &r : o.keys)
            if (r == k) return fail(HE_EINVAL, "%s: gks[%d] is also a key of an RGSW ciphertext", who, i);
    }
    const int N = Q.N, LQ = (int)Q.moduli.size(), levelQ = o.keys[0]->nQk - 1;
    std::vector<uint64_t> s((size_t)n), mono;
    std::vector<int64_t> values;
    std::vector<int32_t> sel((size_t)n);
    auto wipe_host = [&]() {
        Prng::wipe(s.data(), s.size() * 8);
        Prng::wipe(sel.data(), sel.size() * 4);
        if (!values.empty()) Prng::wipe(values.data(), values.size() * 8);
        if (!mono.empty()) Prng::wipe(mono.data(), mono.size() * 8);
    };
    TmpPoly t, pts;  // (cleared before they go back to the pool)
    int rc = t.alloc(hringLWE, 1, 1);
    if (rc == HE_OK) rc = he_intt(hringLWE, 0, hskLWE, t.h);  // :52-53
    if (rc == HE_OK) rc = he_imform(hringLWE, 0, t.h, t.h);
    if (rc == HE_OK) rc = he_poly_download_limb(t.h, 0, 0, s.data());
    if (rc == HE_OK) {
        const uint64_t q0 = rl->moduli[0];
        for (int i = 0; i < n; i++) {  // PolyToBigintCentered (:58), then the map of :66-81 in order of first appearance
            const int64_t v = s[(size_t)i] >= (q0 >> 1) ? (int64_t)(s[(size_t)i] - q0) : (int64_t)s[(size_t)i];
            size_t at = std::find(values.begin(), values.end(), v) - values.begin();
            if (at == values.size()) values.push_back(v);
            sel[(size_t)i] = (int32_t)at;
        }
        const size_t m = values.size();
        mono.assign(m * (size_t)LQ * N, 0);
        for (size_t a = 0; a < m; a++) {  // NewMonomialXi (ring/ring.go:374-396)
            int64_t i = values[a] & (int64_t)mask;
            if (i >= N) i -= (int64_t)2 * N;
            for (int k = 0; k < LQ; k++) {
                uint64_t *row = mono.data() + (a * LQ + k) * (size_t)N;
                if (i < 0) row[N + i] = Q.moduli[(size_t)k] - 1;
                else row[i] = 1;
            }
        }
        rc = pts.alloc(e->hq, LQ, (int)m);
        if (rc == HE_OK) rc = he_poly_upload(pts.h, mono.data(), mono.size());
        if (rc == HE_OK) rc = he_ntt(e->hq, LQ - 1, pts.h, pts.h);       // :78, at the ring's full level
        if (rc == HE_OK) rc = he_mform(e->hq, levelQ, pts.h, pts.h);     // encryptor.go:56, at the ciphertext's
    }
    if (rc == HE_OK) {
        { Scope sc(&e->ctx()); }
        auto p = get<Poly>(pts.h, T_POLY);
        rc = rgsw_encrypt_table(*e, who, o, p->d, p->view().bstride, sel.data(), n);  // :83-89
    }
    wipe_host();
    for (int i = 0; i <= kWindowSize && rc == HE_OK; i++) rc = keygen_galois_key(*kg, who, gal_els[i], o.hskQ, o.hskP, gks[i]);  // :101-105
    const int rs = rlwe_frame_end(e->ctx());
    return rc != HE_OK ? rc : rs;
}

// ---------------------------------------------------------------------------------------
// ring-degree switching and ApplyEvaluationKey (include/hering_ringswitch.h)
// ---------------------------------------------------------------------------------------
// kinds of CO_RING_SWITCH (par[0])
enum { RS_FOLD_NTT = 0, RS_REPLICATE_NTT, RS_STRIDE_DOWN, RS_STRIDE_UP };
// a pair of polynomials of degrees (n, n << log_gap) in either order, n >= 16 (context, batch and limbs: the operand checks)
static int ring_switch_shape(const Poly &a, const Poly &b, int level, int *log_gap, const char *who) {
    const int lo = std::min(a.N, b.N), hi = std::max(a.N, b.N);
    if (lo < 16) return fail(HE_EINVAL, "%s: the small degree %d is below 16", who, lo);
    int lg = 0;
    while ((lo << lg) < hi) lg++;
    if ((lo << lg) != hi) return fail(HE_EINVAL, "%s: degrees %d and %d are not a power-of-two ratio", who, lo, hi);
    if (level < 0 || level >= kMaxLimbs) return fail(HE_EINVAL, "%s: level %d out of range", who, level);
    *log_gap = lg;
    return HE_OK;
}
// MForm(gap^-1 mod q_i) for limbs 0..level of a ring: the fold's per-limb constant
static std::vector<uint64_t> fold_constants(const std::vector<uint64_t> &moduli, int level, int log_gap) {
    std::vector<uint64_t> g((size_t)level + 1);
    for (int i = 0; i <= level; i++) g[i] = to_mont(invmod((1ull << log_gap) % moduli[i], moduli[i]), moduli[i]);
    return g;
}
// the launch of one ring-degree map over B entries (v[0] in, v[1] out); the caller holds the context
static int ring_switch_launch(Ctx &c, const Ring *large, int kind, int level, int log_gap, int n_small, const std::vector<uint64_t> &gapinv,
                              const View *v, int B) {
    const double L = level + 1, NL = (double)((size_t)n_small << log_gap), gap = (double)(1 << log_gap);
    RingSwitchIO io;
    io.in = v[0]; io.out = v[1];
    const LimbTab tab = ident_tab(level + 1);
    if (kind == RS_FOLD_NTT) {
        c.acct(L * (1.0 + 1.0 / gap), 0, B, (int)NL);
        Valu V(large->logN - log_gap);
        V.mul(false, L);  // (one integer Montgomery product per output word, whatever the modulus class)
        V.into(c, B);
        HIP_TRY(launch_ring_degree_fold_ntt(large->dev, tab, gapinv.data(), io, n_small, log_gap, B, c.stream));
    } else if (kind == RS_REPLICATE_NTT) {
        c.acct(L * (1.0 + 1.0 / gap), 0, B, (int)NL);
        HIP_TRY(launch_ring_degree_replicate_ntt(tab, io, n_small, log_gap, B, c.stream));
    } else {
        c.acct(2.0 * L / gap, 0, B, (int)NL);
        HIP_TRY(launch_ring_degree_stride(tab, io, n_small, log_gap, kind == RS_STRIDE_UP, B, c.stream));
    }
    return HE_OK;
}
// A request that addresses a ring alone -- a ring-level map, a step of the ring-packing evaluator: its key (the operation, the
// ring whose tables the launches read or, without one, the context, and par[0..] in order), its launches, and its dispatch over B
// entries.  None of these kernels takes entry tables: a batch is served one by one.
using RingRun = std::function<int(const View *v, int B)>;
static int ring_dispatch(const std::shared_ptr<Ctx> &ctx, CoReq &q, int op, const std::shared_ptr<Ring> &ring,
                         std::initializer_list<int64_t> par, int B, RingRun run) {
    q.op = op; q.obj = ring ? (const void *)ring.get() : (const void *)ctx.get();
    std::copy(par.begin(), par.end(), q.par);
    if (ring) q.keep.push_back(ring);
    q.run = std::move(run);
    q.one_by_one();
    return co_dispatch(*ctx, B, q);
}
// files one ring-level map of in -> out (distinct handles of different degree, named as the entry names them) on the context's queue
static int ring_map_file(const char *who, int op, const std::shared_ptr<Ring> &ring, std::initializer_list<int64_t> par, int level,
                         const std::shared_ptr<Poly> &in, const char *in_name, const std::shared_ptr<Poly> &out, const char *out_name,
                         RingRun run) {
    CoReq q;
    Operands o(q, who, in->ctx, in->N);
    o.in(in, level + 1, in_name);
    o.out(out, level + 1, out_name, Operands::kCall, out->N);
    TRY(o.check());
    return ring_dispatch(in->ctx, q, op, ring, par, in->batch, std::move(run));
}
// one ring-degree map of in -> out
static int ring_switch_file(const char *who, const std::shared_ptr<Ring> &large, int kind, int level, int log_gap,
                            const std::shared_ptr<Poly> &in, const std::shared_ptr<Poly> &out) {
    const std::shared_ptr<Ctx> ctx = in->ctx;
    const int n_small = std::min(in->N, out->N);
    const std::vector<uint64_t> gapinv = kind == RS_FOLD_NTT ? fold_constants(large->moduli, level, log_gap) : std::vector<uint64_t>();
    RingRun run = [ctx, large, kind, level, log_gap, n_small, gapinv](const View *v, int B) -> int {
        return ring_switch_launch(*ctx, large.get(), kind, level, log_gap, n_small, gapinv, v, B);
    };
    return ring_map_file(who, CO_RING_SWITCH, large, {kind, level, log_gap, n_small}, level, in, "in", out, "out", run);
}
int he_map_small_to_large_ntt(he_handle hsmall, he_handle hlarge, int level) {
    GET(ps, Poly, hsmall, T_POLY);
    GET(pl, Poly, hlarge, T_POLY);
    int lg = 0;
    TRY(ring_switch_shape(*ps, *pl, level, &lg, "he_map_small_to_large_ntt"));
    if (ps->N > pl->N) return fail(HE_EINVAL, "he_map_small_to_large_ntt: polSmall (degree %d) is larger than polLarge (%d)", ps->N, pl->N);
    if (lg == 0) return he_poly_copy(hlarge, hsmall, level);
    return ring_switch_file("he_map_small_to_large_ntt", nullptr, RS_REPLICATE_NTT, level, lg, ps, pl);
}
int he_switch_ring_degree_ntt(he_handle hring, int level, he_handle hin, he_handle hout) {
    GET(in, Poly, hin, T_POLY);
    GET(out, Poly, hout, T_POLY);
    int lg = 0;
    TRY(ring_switch_shape(*in, *out, level, &lg, "he_switch_ring_degree_ntt"));
    std::shared_ptr<Ring> r;
    if (hring || in->N > out->N) {
        r = get<Ring>(hring, T_RING);
        if (!r) return fail(HE_EHANDLE, "he_switch_ring_degree_ntt: bad ring handle %llu (required for large -> small)", (unsigned long long)hring);
        if (r->ctx != in->ctx) return fail(HE_EINVAL, "he_switch_ring_degree_ntt: the ring belongs to another context");
        if (r->N != std::max(in->N, out->N)) return fail(HE_EINVAL, "he_switch_ring_degree_ntt: ring degree %d != the large degree %d", r->N, std::max(in->N, out->N));
        if (level >= r->nmod()) return fail(HE_EINVAL, "he_switch_ring_degree_ntt: level %d out of range [0,%d]", level, r->nmod() - 1);
    }
    if (lg == 0) return he_poly_copy(hout, hin, level);
    if (in->N > out->N) return ring_switch_file("he_switch_ring_degree_ntt", r, RS_FOLD_NTT, level, lg, in, out);
    return ring_switch_file("he_switch_ring_degree_ntt", nullptr, RS_REPLICATE_NTT, level, lg, in, out);
}
int he_switch_ring_degree(int level, he_handle hin, he_handle hout) {
    GET(in, Poly, hin, T_POLY);
    GET(out, Poly, hout, T_POLY);
    int lg = 0;
    TRY(ring_switch_shape(*in, *out, level, &lg, "he_switch_ring_degree"));
    if (lg == 0) return he_poly_copy(hout, hin, level);
    return ring_switch_file("he_switch_ring_degree", nullptr, in->N > out->N ? RS_STRIDE_DOWN : RS_STRIDE_UP, level, lg, in, out);
}

// One key switch at the evaluator's degree N composed with one ring map over both components (2B entries in one launch, the
// map's io.zsplit = B): the degree-changing forms of ApplyEvaluationKey, the DomainSwitcher, and ring packing's Split and Merge.
// Both components at degree N are staged in scratch as [2][B] entries, t0 then t1: this reserves the key switch's scratch (2 L in,
// 2 L out, key) plus the staged pair, and hands the pair back.
static int ks_staged_begin(Evaluator &ev, const Evk &k, int level, int B, View *t0, View *t1) {
    BasisExtender &be = *ev.be;
    const size_t sQ = (size_t)(level + 1) * be.Q->N, wQ = (size_t)B * sQ;
    TRY(keyswitch_begin(ev, k, level, 4.0 * (level + 1), true, B, 2 * wQ + 2));
    uint64_t *t = be.ctx->arena_take(2 * wQ);
    *t0 = View{t, sQ}; *t1 = View{t + wQ, sQ};
    return HE_OK;
}
using StagedMap = std::function<int(const View &t0, const View &t1)>;  // the map's accounting and launch, from or into the staged pair
// GadgetProduct(operand) with `addend` in the ModDown epilogue of component 0, into (t0, t1); then map(t0, t1) to the caller's outputs
static int key_switch_then_map(Evaluator &ev, const Evk &k, int level, int B, const View &addend, const View &operand, const StagedMap &map) {
    View t0{nullptr, 0}, t1{nullptr, 0};
    TRY(ks_staged_begin(ev, k, level, B, &t0, &t1));
    TRY(key_switch(ev, KS_GADGET_PRODUCT, level, k, KsAlias{}, GpArgs{&operand, nullptr, t0, t1, B, &addend}));
    return map(t0, t1);
}
// map(t0, t1) from the caller's inputs; then GadgetProduct(t1) with t0 as the addend, into (out0, out1)
static int map_then_key_switch(Evaluator &ev, const Evk &k, int level, int B, const StagedMap &map, const View &out0, const View &out1) {
    View t0{nullptr, 0}, t1{nullptr, 0};
    TRY(ks_staged_begin(ev, k, level, B, &t0, &t1));
    TRY(map(t0, t1));
    return key_switch(ev, KS_GADGET_PRODUCT, level, k, KsAlias{}, GpArgs{&t1, nullptr, out0, out1, B, &t0});
}

// ApplyEvaluationKey (core/rlwe/evaluator_evaluationkey.go:36-106): out0 = in0 + GadgetProduct(in1)_0, out1 = GadgetProduct(in1)_1
// (applyEvaluationKey, :98-106) as ONE key switch with the Add in its ModDown epilogue; the degree-changing forms add the ring map
// of the reference after (large -> small: the fold of both components, one launch over 2B entries) or before it (small -> large:
// the replication of both components into scratch at N, then the key switch with the replicated in0 as the addend).
enum { AEK_SAME = 0, AEK_DOWN, AEK_UP };
int he_apply_evaluation_key(he_handle hev, int level, he_handle hin0, he_handle hin1, he_handle hk, he_handle hout0, he_handle hout1) {
    static const char *who = "he_apply_evaluation_key";
    GET(ev, Evaluator, hev, T_EVAL);
    GET(in0, Poly, hin0, T_POLY);
    GET(in1, Poly, hin1, T_POLY);
    GET(k, Evk, hk, T_EVK);
    GET(out0, Poly, hout0, T_POLY);
    GET(out1, Poly, hout1, T_POLY);
    BasisExtender &be = *ev->be;
    TRY(check_key(*ev, *k, level, who));
    const int N = be.Q->N, Nin = in0->N, Nout = out0->N;
    if (in1->N != Nin || out1->N != Nout) return fail(HE_EINVAL, "%s: the two components of a ciphertext differ in degree", who);
    // the reference's errors (:51-53, :68-70): the large side must be the evaluator's degree
    if (Nin < Nout && Nout != N) return fail(HE_EINVAL, "%s: opOut ring degree does not match evaluator params ring degree", who);
    if (Nin > Nout && Nin != N) return fail(HE_EINVAL, "%s: ctIn ring degree does not match evaluator params ring degree", who);
    // same degree: both sides are the evaluator's degree (the key switch runs at N over every operand)
    if (Nin == Nout && Nin != N) return fail(HE_EINVAL, "%s: ciphertext ring degree %d does not match evaluator params ring degree %d", who, Nin, N);
    const int form = Nin == Nout ? AEK_SAME : (Nin > Nout ? AEK_DOWN : AEK_UP);
    int lg = 0;
    if (form != AEK_SAME) TRY(ring_switch_shape(*in0, *out0, level, &lg, who));
    CoReq q;
    Operands o(q, who, be);
    const int i0 = o.in(in0, level + 1, "in0", Operands::kCall, Nin), i1 = o.in(in1, level + 1, "in1", Operands::kCall, Nin);
    const int o0 = o.out(out0, level + 1, "out0", Operands::kCall, Nout), o1 = o.out(out1, level + 1, "out1", Operands::kCall, Nout);
    o.all_inplace = true;  // (handles of different degree never coincide; at equal degree any output may be any input, out0 != out1)
    TRY(o.check());
    // as in he_relinearize: an output that is the key switch's operand (in1) or the OTHER component's addend (in0 == out1) cannot be
    // batched; the crossed case stages the addend first (component 1's epilogue would overwrite it before component 0 reads it)
    const bool cross = o.same(i0, o1);
    KsAlias alias;  // (of the key switch proper: the degree-changing forms run it on scratch)
    if (form == AEK_SAME) { alias.out_is_operand = o.same(i1, o0) || o.same(i1, o1); alias.crossed = cross; }
    const int n_small = std::min(Nin, Nout);
    const std::vector<uint64_t> gapinv = form == AEK_DOWN ? fold_constants(be.Q->moduli, level, lg) : std::vector<uint64_t>();
    ks_request(q, CO_APPLY_EVK, ev, k, level, form == AEK_SAME ? KS_GADGET_PRODUCT : KS_FORM_COUNT, alias); q.par[1] = form; q.par[2] = lg;
    if (form == AEK_SAME) q.run = [ev, k, level, cross, alias](const View *v, int B) -> int {
        BasisExtender &be = *ev->be;
        const size_t sQ = (size_t)(level + 1) * be.Q->N, wQ = (size_t)B * sQ;
        // the key switch: 2 L in, 2 L out, key; its scratch and the staged addend
        TRY(keyswitch_begin(*ev, *k, level, 4.0 * (level + 1), true, B, cross ? wQ + 2 : 0));
        hipStream_t st = be.ctx->stream;
        View a0 = v[0];
        if (cross) {  // (served one by one: plain views)
            a0 = View{be.ctx->arena_take(wQ), sQ};
            HIP_TRY(launch_ew(be.qp, ident_tab(level + 1), EW_COPY, v[0], v[0], a0, B, nullptr, nullptr, st));
        }
        return key_switch(*ev, KS_GADGET_PRODUCT, level, *k, alias, GpArgs{&v[1], nullptr, v[2], v[3], B, &a0});
    };
    // the degree-changing forms: the fold of the key switch's result (down) or the replication of its input (up)
    else q.run = [ev, k, level, form, lg, n_small, gapinv](const View *v, int B) -> int {
        BasisExtender &be = *ev->be;
        hipStream_t st = be.ctx->stream;
        const bool up = form == AEK_UP;
        auto map = [&](const View &t0, const View &t1) -> int {
            RingSwitchIO io;
            io.zsplit = B;
            if (up) { io.in = v[0]; io.in2 = v[1]; io.out = t0; io.out2 = t1; }
            else { io.in = t0; io.in2 = t1; io.out = v[2]; io.out2 = v[3]; }
            be.ctx->acct(2.0 * (level + 1) * (1.0 + 1.0 / (1 << lg)), 0, B, be.Q->N);
            if (up) HIP_TRY(launch_ring_degree_replicate_ntt(ident_tab(level + 1), io, n_small, lg, 2 * B, st));
            else {
                Valu V(be.Q->logN - lg); V.mul(false, 2.0 * (level + 1)); V.into(*be.ctx, B);  // (integer products on every limb)
                HIP_TRY(launch_ring_degree_fold_ntt(be.Q->dev, ident_tab(level + 1), gapinv.data(), io, n_small, lg, 2 * B, st));
            }
            return HE_OK;
        };
        return up ? map_then_key_switch(*ev, *k, level, B, map, v[2], v[3]) : key_switch_then_map(*ev, *k, level, B, v[0], v[1], map);
    };
    // (the ring maps of the degree-changing forms take no entry tables)
    if (form != AEK_SAME) q.one_by_one();
    return co_dispatch(*be.ctx, o.B, q);
}

// ---------------------------------------------------------------------------------------
// the CKKS DomainSwitcher (include/hering_bridge.h; schemes/ckks/bridge.go, ring/conjugate_invariant.go)
// ---------------------------------------------------------------------------------------
// kinds of CO_CI_BRIDGE / CO_CI_BRIDGE_CT (par[1])
enum { BR_FOLD = 0, BR_UNFOLD };
// one launch covers every entry of both components in its grid's z dimension (the DomainSwitcher and ring packing alike)
constexpr int kMaxZEntries = 65535;
static int z_entries(long entries, const char *who) {
    if (entries > kMaxZEntries)
        return fail(HE_EINVAL, "%s: %ld entries in one call, at most %d (split the batch)", who, entries, kMaxZEntries);
    return HE_OK;
}
// a standard polynomial of degree 2n and a conjugate-invariant one of degree n >= 16 (context, batch and limbs: the operand checks)
static int bridge_shape(const Poly &std_, const Poly &ci, int level, const char *who, const char *ratio_msg) {
    if (std_.N != 2 * ci.N) return fail(HE_EINVAL, "%s: %s (%d and %d)", who, ratio_msg, std_.N, ci.N);
    if (ci.N < 16) return fail(HE_EINVAL, "%s: the small degree %d is below 16", who, ci.N);
    if (level < 0 || level >= kMaxLimbs) return fail(HE_EINVAL, "%s: level %d out of range", who, level);
    return z_entries(2L * std_.batch, who);
}
// one bridge map of in -> out
static int bridge_file(const char *who, const std::shared_ptr<Ring> &moduli, int kind, int level, const std::shared_ptr<Poly> &in,
                       const std::shared_ptr<Poly> &out) {
    const std::shared_ptr<Ctx> ctx = in->ctx;
    const int n = std::min(in->N, out->N);
    RingRun run = [ctx, moduli, kind, level, n](const View *v, int B) -> int {
        RingSwitchIO io;
        io.in = v[0]; io.out = v[1];
        ctx->acct(1.5 * (level + 1), 0, B, 2 * n);  // (every input word read once, every output word written once)
        if (kind == BR_FOLD) HIP_TRY(launch_ci_bridge_fold(moduli->dev, ident_tab(level + 1), io, n, B, ctx->stream));
        else HIP_TRY(launch_ci_bridge_unfold(ident_tab(level + 1), io, n, B, ctx->stream));
        return HE_OK;
    };
    const char *std_name = "polyStandard", *ci_name = "polyConjugateInvariant";
    return ring_map_file(who, CO_CI_BRIDGE, moduli, {level, kind, n}, level, in, kind == BR_FOLD ? std_name : ci_name, out,
                         kind == BR_FOLD ? ci_name : std_name, run);
}
int he_unfold_conjugate_invariant_to_standard(int level, he_handle hci, he_handle hstd) {
    static const char *who = "he_unfold_conjugate_invariant_to_standard";
    GET(ci, Poly, hci, T_POLY);
    GET(st, Poly, hstd, T_POLY);
    TRY(bridge_shape(*st, *ci, level, who, "ring degree of polyStandard must be twice the ring degree of polyConjugateInvariant"));
    return bridge_file(who, nullptr, BR_UNFOLD, level, ci, st);
}
int he_fold_standard_to_conjugate_invariant(he_handle hring, int level, he_handle hstd, he_handle hci) {
    static const char *who = "he_fold_standard_to_conjugate_invariant";
    GET(r, Ring, hring, T_RING);
    GET(st, Poly, hstd, T_POLY);
    GET(ci, Poly, hci, T_POLY);
    TRY(bridge_shape(*st, *ci, level, who, "ring degree of polyStandard must be 2N and ring degree of polyConjugateInvariant must be N"));
    if (r->ctx != st->ctx) return fail(HE_EINVAL, "%s: the ring belongs to another context", who);
    if (r->N != st->N && r->N != ci->N) return fail(HE_EINVAL, "%s: ring degree %d is neither %d nor %d", who, r->N, ci->N, st->N);
    if (level >= r->nmod()) return fail(HE_EINVAL, "%s: level %d out of range [0,%d]", who, level, r->nmod() - 1);
    return bridge_file(who, r, BR_FOLD, level, st, ci);
}
// ComplexToReal (bridge.go:57-95): GadgetProduct(in1) with in0 as the ModDown epilogue's addend, into scratch at N, then the fold of
// both components in one launch over 2B entries.  RealToComplex (bridge.go:104-144): the unfold of both components into scratch at
// N in one launch, then the key switch of the unfolded in1 with the unfolded in0 as the addend (the reference unfolds into opOut and
// adds there: the same words, ringQ.Add being symmetric).
static int bridge_ct(const char *who, int kind, he_handle hev, int level, he_handle hin0, he_handle hin1, he_handle hk, he_handle hout0,
                     he_handle hout1) {
    const auto ev = get<Evaluator>(hev, T_EVAL);
    const auto k = get<Evk>(hk, T_EVK);
    const auto in0 = get<Poly>(hin0, T_POLY), in1 = get<Poly>(hin1, T_POLY), out0 = get<Poly>(hout0, T_POLY), out1 = get<Poly>(hout1, T_POLY);
    if (!ev) return fail(HE_EHANDLE, "%s: bad Evaluator handle %llu", who, (unsigned long long)hev);
    if (!k) return fail(HE_EHANDLE, "%s: bad Evk handle %llu", who, (unsigned long long)hk);
    if (!in0 || !in1 || !out0 || !out1) return fail(HE_EHANDLE, "%s: bad Poly handle", who);
    BasisExtender &be = *ev->be;
    const char *name = kind == BR_FOLD ? "ComplexToReal" : "RealToComplex";
    if (be.type != 0) return fail(HE_EINVAL, "%s: cannot %s: provided evaluator is not instantiated with RingType ring.Standard", who, name);
    TRY(check_key(*ev, *k, level, who));
    const int N = be.Q->N, Nin = in0->N, Nout = out0->N;
    if (in1->N != Nin || out1->N != Nout) return fail(HE_EINVAL, "%s: the two components of a ciphertext differ in degree", who);
    if (kind == BR_FOLD && Nin != 2 * Nout) return fail(HE_EINVAL, "%s: cannot ComplexToReal: ctIn ring degree must be twice opOut ring degree", who);
    if (kind == BR_UNFOLD && 2 * Nin != Nout) return fail(HE_EINVAL, "%s: cannot RealToComplex: opOut ring degree must be twice ctIn ring degree", who);
    if (std::max(Nin, Nout) != N)
        return fail(HE_EINVAL, "%s: %s ring degree does not match evaluator params ring degree", who, kind == BR_FOLD ? "ctIn" : "opOut");
    TRY(bridge_shape(kind == BR_FOLD ? *in0 : *out0, kind == BR_FOLD ? *out0 : *in0, level, who, "degrees are not N and N/2"));
    CoReq q;
    Operands o(q, who, be);
    o.in(in0, level + 1, "in0", Operands::kCall, Nin); o.in(in1, level + 1, "in1", Operands::kCall, Nin);
    o.out(out0, level + 1, "out0", Operands::kCall, Nout); o.out(out1, level + 1, "out1", Operands::kCall, Nout);
    TRY(o.check());  // (handles of different degree never coincide: only out0 == out1 can, and is rejected)
    const int n = N / 2;
    // (the key switch runs on scratch on one side: none of its outputs is its operand)
    ks_request(q, CO_CI_BRIDGE_CT, ev, k, level, KS_FORM_COUNT, KsAlias{}); q.par[1] = kind;
    q.run = [ev, k, level, kind, n](const View *v, int B) -> int {
        BasisExtender &be = *ev->be;
        hipStream_t st = be.ctx->stream;
        const bool unfold = kind == BR_UNFOLD;
        auto map = [&](const View &t0, const View &t1) -> int {
            RingSwitchIO io;
            io.zsplit = B;
            if (unfold) { io.in = v[0]; io.in2 = v[1]; io.out = t0; io.out2 = t1; }
            else { io.in = t0; io.in2 = t1; io.out = v[2]; io.out2 = v[3]; }
            be.ctx->acct(2.0 * 1.5 * (level + 1), 0, B, be.Q->N);
            if (unfold) HIP_TRY(launch_ci_bridge_unfold(ident_tab(level + 1), io, n, 2 * B, st));
            else HIP_TRY(launch_ci_bridge_fold(be.Q->dev, ident_tab(level + 1), io, n, 2 * B, st));
            return HE_OK;
        };
        return unfold ? map_then_key_switch(*ev, *k, level, B, map, v[2], v[3]) : key_switch_then_map(*ev, *k, level, B, v[0], v[1], map);
    };
    q.one_by_one();  // (the ring maps take no entry tables)
    return co_dispatch(*be.ctx, o.B, q);
}
int he_complex_to_real(he_handle ev, int level, he_handle in0, he_handle in1, he_handle evk, he_handle out0, he_handle out1) {
    return bridge_ct("he_complex_to_real", BR_FOLD, ev, level, in0, in1, evk, out0, out1);
}
int he_real_to_complex(he_handle ev, int level, he_handle in0, he_handle in1, he_handle evk, he_handle out0, he_handle out1) {
    return bridge_ct("he_real_to_complex", BR_UNFOLD, ev, level, in0, in1, evk, out0, out1);
}

// ---------------------------------------------------------------------------------------
// the ring-packing evaluator (include/hering_ringpack.h; core/rlwe/ring_packing.go)
// ---------------------------------------------------------------------------------------
// Every entry is filed on the queue and served one by one (none of the kernels takes entry tables, as the ring maps).
static int rp_ring(const Ring &r, int level, const char *who) {
    if (r.type != 0) return fail(HE_EINVAL, "%s: method is only supported for ring.Type = ring.Standard", who);
    if (level < 0 || level >= r.nmod() || level >= kMaxLimbs) return fail(HE_EINVAL, "%s: level %d out of range [0,%d]", who, level, r.nmod() - 1);
    return HE_OK;
}
int he_ring_xpow2_ntt(he_handle hring, int level, int i, int div, he_handle hout) {
    static const char *who = "he_ring_xpow2_ntt";
    GET(r, Ring, hring, T_RING);
    GET(out, Poly, hout, T_POLY);
    TRY(rp_ring(*r, level, who));
    if (r->N < 16) return fail(HE_EINVAL, "%s: ring degree %d is below 16", who, r->N);
    if (i < 0 || i >= r->logN) return fail(HE_EINVAL, "%s: i = %d out of range [0,%d]", who, i, r->logN - 1);
    TRY(z_entries(out->batch, who));
    const std::shared_ptr<Ctx> ctx = r->ctx;
    CoReq q;
    Operands o(q, who, *r);
    o.out(out, level + 1, "out");
    TRY(o.check());
    RingRun run = [ctx, r, level, i, div](const View *v, int B) -> int {
        ctx->acct(level + 1, 0, B, r->N);
        HIP_TRY(launch_xpow2_fill(r->dev, v[0], i, div != 0, level + 1, B, ctx->stream));
        return HE_OK;
    };
    return ring_dispatch(ctx, q, CO_RING_PACK, r, {RP_XPOW2, level, i, div != 0}, out->batch, run);
}
// the launch of Split's (RP_SPLIT) or Merge's (RP_MERGE) ring map over B entries per component (ncomp components); the caller
// holds the context.  (The two launches are spelled out: a device error's message names the call that failed.)
static int rp_halves_launch(int kind, Ctx &c, const Ring &large, const RingPackIO &io, bool odd, int level, int B, int ncomp) {
    c.acct(ncomp * (level + 1) * (odd ? 2.0 : 1.5), odd ? 0.5 * (level + 1) : 0.0, B, large.N);
    if (odd) { Valu V(large.logN - 1); V.mul(false, (double)ncomp * (level + 1)); V.into(c, B); }
    if (kind == RP_MERGE) HIP_TRY(launch_ring_merge(large.dev, io, level + 1, ncomp * B, c.stream));
    else HIP_TRY(launch_ring_split(large.dev, io, level + 1, ncomp * B, c.stream));
    return HE_OK;
}
int he_ring_split_ntt(he_handle hring, int level, he_handle hin, he_handle heven, he_handle hodd) {
    static const char *who = "he_ring_split_ntt";
    GET(r, Ring, hring, T_RING);
    GET(in, Poly, hin, T_POLY);
    TRY(rp_ring(*r, level, who));
    if (r->N / 2 < 16) return fail(HE_EINVAL, "%s: the small degree %d is below 16", who, r->N / 2);
    const int B = in->batch;
    TRY(z_entries(B, who));
    CoReq q;
    Operands o(q, who, *r);
    o.in(in, level + 1, "in");
    o.out(heven, level + 1, "outEven", B, r->N / 2);
    o.out(o.opt(hodd), level + 1, "outOdd", B, r->N / 2);
    TRY(o.check());
    const bool has_odd = hodd != 0;
    RingRun run = [r, level, has_odd](const View *v, int B) -> int {
        RingPackIO io;
        io.x[0] = v[0]; io.o[0] = v[1]; io.p[0] = v[2];
        return rp_halves_launch(RP_SPLIT, *r->ctx, *r, io, has_odd, level, B, 1);
    };
    return ring_dispatch(r->ctx, q, CO_RING_PACK, r, {RP_SPLIT, level, has_odd}, B, run);
}
int he_ring_merge_ntt(he_handle hring, int level, he_handle heven, he_handle hodd, he_handle hout) {
    static const char *who = "he_ring_merge_ntt";
    GET(r, Ring, hring, T_RING);
    GET(out, Poly, hout, T_POLY);
    TRY(rp_ring(*r, level, who));
    if (r->N / 2 < 16) return fail(HE_EINVAL, "%s: the small degree %d is below 16", who, r->N / 2);
    const int B = out->batch;
    TRY(z_entries(B, who));
    CoReq q;
    Operands o(q, who, *r, B);
    o.in(heven, level + 1, "inEven", B, r->N / 2);
    o.in(o.opt(hodd), level + 1, "inOdd", B, r->N / 2);
    o.out(out, level + 1, "out");
    TRY(o.check());
    const bool has_odd = hodd != 0;
    RingRun run = [r, level, has_odd](const View *v, int B) -> int {
        RingPackIO io;
        io.x[0] = v[0]; io.y[0] = v[1]; io.o[0] = v[2];
        return rp_halves_launch(RP_MERGE, *r->ctx, *r, io, has_odd, level, B, 1);
    };
    return ring_dispatch(r->ctx, q, CO_RING_PACK, r, {RP_MERGE, level, has_odd}, B, run);
}
// the shared checks of he_ringpack_split / he_ringpack_merge on the evaluator, the key and the odd halves' handles; B entries per operand
static int rp_ct_checks(const Evaluator &ev, const Evk &k, int &level, int B, he_handle ho0, he_handle ho1, const char *who) {
    const BasisExtender &be = *ev.be;
    if (be.type != 0) return fail(HE_EINVAL, "%s: method is only supported for ring.Type = ring.Standard", who);
    const int asked = level;
    TRY(check_key(ev, k, level, who));
    if (level != asked) return fail(HE_EINVAL, "%s: the key has %d Q limbs, level %d needs %d", who, k.nQk, asked, asked + 1);
    if (level >= be.LQ || level >= kMaxLimbs) return fail(HE_EINVAL, "%s: level %d out of range [0,%d]", who, level, be.LQ - 1);
    TRY(z_entries(2L * B, who));
    if (be.Q->N / 2 < 16) return fail(HE_EINVAL, "%s: the small degree %d is below 16", who, be.Q->N / 2);
    if ((ho0 == 0) != (ho1 == 0)) return fail(HE_EINVAL, "%s: odd0 and odd1 are both given or both 0", who);
    return HE_OK;
}
int he_ringpack_split(he_handle hev, int level, he_handle hin0, he_handle hin1, he_handle hk, he_handle he0, he_handle he1, he_handle ho0,
                      he_handle ho1) {
    static const char *who = "he_ringpack_split";
    GET(ev, Evaluator, hev, T_EVAL);
    GET(in0, Poly, hin0, T_POLY);
    GET(k, Evk, hk, T_EVK);
    const int B = in0->batch;
    TRY(rp_ct_checks(*ev, *k, level, B, ho0, ho1, who));
    BasisExtender &be = *ev->be;
    const int n = be.Q->N / 2;
    CoReq q;
    Operands o(q, who, be);
    o.in(in0, level + 1, "ctN[0]");
    o.in(hin1, level + 1, "ctN[1]");
    o.out(he0, level + 1, "even0", B, n);
    o.out(he1, level + 1, "even1", B, n);
    o.out(o.opt(ho0), level + 1, "odd0", B, n);
    o.out(o.opt(ho1), level + 1, "odd1", B, n);
    TRY(o.check());
    const bool has_odd = ho0 != 0;
    ks_request(q, CO_RINGPACK_CT, ev, k, level, KS_FORM_COUNT, KsAlias{}); q.par[1] = 0; q.par[2] = has_odd;
    q.run = [ev, k, level, has_odd](const View *v, int B) -> int {
        auto map = [&](const View &t0, const View &t1) {
            RingPackIO io;
            io.zsplit = B;
            io.x[0] = t0; io.x[1] = t1; io.o[0] = v[2]; io.o[1] = v[3]; io.p[0] = v[4]; io.p[1] = v[5];
            return rp_halves_launch(RP_SPLIT, *ev->be->ctx, *ev->be->Q, io, has_odd, level, B, 2);
        };
        return key_switch_then_map(*ev, *k, level, B, v[0], v[1], map);
    };
    q.one_by_one();
    return co_dispatch(*be.ctx, B, q);
}
int he_ringpack_merge(he_handle hev, int level, he_handle he0, he_handle he1, he_handle ho0, he_handle ho1, he_handle hk, he_handle hout0,
                      he_handle hout1) {
    static const char *who = "he_ringpack_merge";
    GET(ev, Evaluator, hev, T_EVAL);
    GET(k, Evk, hk, T_EVK);
    GET(out0, Poly, hout0, T_POLY);
    const int B = out0->batch;
    TRY(rp_ct_checks(*ev, *k, level, B, ho0, ho1, who));
    BasisExtender &be = *ev->be;
    const int n = be.Q->N / 2;
    CoReq q;
    Operands o(q, who, be, B);
    o.in(he0, level + 1, "even0", B, n);
    o.in(he1, level + 1, "even1", B, n);
    o.in(o.opt(ho0), level + 1, "odd0", B, n);
    o.in(o.opt(ho1), level + 1, "odd1", B, n);
    o.out(out0, level + 1, "ctN[0]");
    o.out(hout1, level + 1, "ctN[1]");
    TRY(o.check());
    const bool has_odd = ho0 != 0;
    ks_request(q, CO_RINGPACK_CT, ev, k, level, KS_FORM_COUNT, KsAlias{}); q.par[1] = 1; q.par[2] = has_odd;
    q.run = [ev, k, level, has_odd](const View *v, int B) -> int {
        auto map = [&](const View &t0, const View &t1) {
            RingPackIO io;
            io.zsplit = B;
            io.x[0] = v[0]; io.x[1] = v[1]; io.y[0] = v[2]; io.y[1] = v[3]; io.o[0] = t0; io.o[1] = t1;
            return rp_halves_launch(RP_MERGE, *ev->be->ctx, *ev->be->Q, io, has_odd, level, B, 2);
        };
        return map_then_key_switch(*ev, *k, level, B, map, v[4], v[5]);
    };
    q.one_by_one();
    return co_dispatch(*be.ctx, B, q);
}
int he_ringpack_expand_step(he_handle hring, int level, int k, int sum_only, he_handle hin0, he_handle hin1, he_handle htmp0, he_handle htmp1,
                            he_handle hout0, he_handle hout1) {
    static const char *who = "he_ringpack_expand_step";
    GET(r, Ring, hring, T_RING);
    GET(in0, Poly, hin0, T_POLY);
    TRY(rp_ring(*r, level, who));
    if (r->N < 16) return fail(HE_EINVAL, "%s: ring degree %d is below 16", who, r->N);
    if (k < 0 || k >= r->logN) return fail(HE_EINVAL, "%s: k = %d out of range [0,%d]", who, k, r->logN - 1);
    const int m = in0->batch;
    TRY(z_entries(2L * m, who));
    const bool so = sum_only != 0;
    CoReq q;
    Operands o(q, who, *r);
    const int i0 = o.in(in0, level + 1, "in0"), i1 = o.in(hin1, level + 1, "in1");
    o.in(htmp0, level + 1, "tmp0");
    o.in(htmp1, level + 1, "tmp1");
    const int o0 = o.out(hout0, level + 1, "out0", so ? m : 2 * m), o1 = o.out(hout1, level + 1, "out1", so ? m : 2 * m);
    if (so) { o.inplace(o0, i0); o.inplace(o1, i1); }
    TRY(o.check());
    const std::shared_ptr<Ctx> ctx = r->ctx;
    RingRun run = [ctx, r, level, k, so](const View *v, int B) -> int {
        RingPackIO io;
        io.zsplit = B;
        io.x[0] = v[0]; io.x[1] = v[1]; io.y[0] = v[2]; io.y[1] = v[3]; io.o[0] = v[4]; io.o[1] = v[5];
        ctx->acct(2.0 * (level + 1) * (so ? 3.0 : 4.0), 0, B, r->N);
        if (!so) { Valu V(r->logN); V.mul(false, 2.0 * (level + 1)); V.into(*ctx, B); }
        HIP_TRY(launch_expand_step(r->dev, io, k, B, so, level + 1, 2 * B, ctx->stream));
        return HE_OK;
    };
    // (the second half of out lies m entries past the first: a request is its whole batch, whatever the queue's limit)
    return ring_dispatch(ctx, q, CO_RING_PACK, r, {RP_EXPAND, level, k, so}, m, run);
}
// the operands of a pack step: count pairs of single ciphertexts and T; fills the request (operands 4 z + {0, 1, 2, 3} = a0, a1, b0,
// b1 of pair z, then t0, t1) and counts the pairs by kind
static int rp_pack_operands(const char *who, const Ring &r, int level, int count, const he_handle *a0, const he_handle *a1, const he_handle *b0,
                            const he_handle *b1, he_handle ht0, he_handle ht1, CoReq &q, int kinds[3]) {
    TRY(rp_ring(r, level, who));
    if (r.N < 16) return fail(HE_EINVAL, "%s: ring degree %d is below 16", who, r.N);
    if (count < 1) return fail(HE_EINVAL, "%s: count = %d, at least one pair is needed", who, count);
    TRY(z_entries(2L * count, who));
    if (!a0 || !a1 || !b0 || !b1) return fail(HE_EINVAL, "%s: null handle array", who);
    // No handle may occur twice among the operands, whatever the step does with each: this call's own identity rule, held with a
    // set (a step takes thousands of pairs; the pairwise rule of reject_aliasing is for the handful of operands of other calls),
    // so the operands are declared as read.
    Operands o(q, who, r);
    std::unordered_set<const uint64_t *> seen;
    auto once = [&](int i) { return !o.ops[i].p || seen.insert(o.ops[i].p->d).second; };
    kinds[0] = kinds[1] = kinds[2] = 0;
    const he_handle *hs[4] = {a0, a1, b0, b1};
    for (int z = 0; z < count; z++) {
        if ((a0[z] == 0) != (a1[z] == 0) || (b0[z] == 0) != (b1[z] == 0))
            return fail(HE_EINVAL, "%s: pair %d: the two components of a ciphertext are both given or both 0", who, z);
        if (!a0[z] && !b0[z]) return fail(HE_EINVAL, "%s: pair %d is empty", who, z);
        kinds[a0[z] && b0[z] ? 0 : (a0[z] ? 1 : 2)]++;
        for (int s = 0; s < 4; s++)
            if (!once(o.in(o.opt(hs[s][z]), level + 1, "a / b", 1))) return fail(HE_EINVAL, "%s: a handle occurs twice among the operands (pair %d)", who, z);
    }
    for (he_handle ht : {ht0, ht1})
        if (!once(o.in(ht, level + 1, "t0 / t1", count))) return fail(HE_EINVAL, "%s: a handle occurs twice among the operands (t0 / t1)", who);
    return o.check();
}
static int rp_pack_step(const char *who, he_handle hring, int level, int k, bool post, int count, const he_handle *a0, const he_handle *a1,
                        const he_handle *b0, const he_handle *b1, he_handle ht0, he_handle ht1) {
    std::shared_ptr<Ring> r = get<Ring>(hring, T_RING);
    if (!r) return fail(HE_EHANDLE, "%s: bad Ring handle %llu", who, (unsigned long long)hring);
    CoReq q;
    int kinds[3];
    TRY(rp_pack_operands(who, *r, level, count, a0, a1, b0, b1, ht0, ht1, q, kinds));
    if (!post && (k < 0 || k >= r->logN)) return fail(HE_EINVAL, "%s: k = %d out of range [0,%d]", who, k, r->logN - 1);
    const std::shared_ptr<Ctx> ctx = r->ctx;
    // polynomial limbs moved per component and limb: pre -- both: a, b in, a, T out; one: 1 in, T out (+ b out); post -- 2 in, 1 out
    const double words = post ? 3.0 * count : 4.0 * kinds[0] + 2.0 * kinds[1] + 3.0 * kinds[2];
    const double muls = post ? 0.0 : (double)(kinds[0] + kinds[2]);
    RingRun run = [ctx, r, level, k, post, count, words, muls](const View *v, int) -> int {
        // the addresses of the pairs' polynomials, rows [a0 | a1 | b0 | b1]: a device table in scratch, filled from kernel arguments
        std::vector<size_t> tab(4 * (size_t)count);
        for (int z = 0; z < count; z++)
            for (int s = 0; s < 4; s++) tab[(size_t)s * count + z] = (size_t)(uintptr_t)v[4 * z + s].p;
        size_t *d = nullptr;
        TRY(scratch_words(*ctx, tab, &d));
        ctx->acct(2.0 * (level + 1) * words, 0, 1, r->N);
        if (muls > 0) { Valu V(r->logN); V.mul(false, 2.0 * (level + 1) * muls); V.into(*ctx, 1); }
        HIP_TRY(launch_pack_step(r->dev, reinterpret_cast<const uint64_t *>(d), v[4 * count], v[4 * count + 1], k, post, count, 2.0 * words,
                                 level + 1, ctx->stream));
        return HE_OK;
    };
    return ring_dispatch(ctx, q, CO_RING_PACK, r, {post ? RP_PACK_POST : RP_PACK_PRE, level, k, count}, 1, run);
}
int he_ringpack_pack_pre(he_handle ring, int level, int k, int count, const he_handle *a0, const he_handle *a1, const he_handle *b0,
                         const he_handle *b1, he_handle t0, he_handle t1) {
    return rp_pack_step("he_ringpack_pack_pre", ring, level, k, false, count, a0, a1, b0, b1, t0, t1);
}
int he_ringpack_pack_post(he_handle ring, int level, int count, const he_handle *a0, const he_handle *a1, const he_handle *b0,
                          const he_handle *b1, he_handle t0, he_handle t1) {
    return rp_pack_step("he_ringpack_pack_post", ring, level, 0, true, count, a0, a1, b0, b1, t0, t1);
}

// ---------------------------------------------------------------------------------------
// RGSW external product (include/hering_rgsw.h; core/rgsw/evaluator.go)
// ---------------------------------------------------------------------------------------
namespace {
// What a select form indexes: the keys of one evaluator and shape, with a resident [2][n] device table of addresses (row 0: the
// keys' words; row 1: the set's own)
struct KeySet : Obj {
    std::shared_ptr<Evaluator> ev;
    size_t *d_tab = nullptr;
    using Obj::Obj;
    int upload(const std::vector<size_t> &rows) {  // (the caller holds the context)
        HIP_TRY(hipMalloc((void **)&d_tab, rows.size() * sizeof(size_t)));
        HIP_TRY(hipMemcpy(d_tab, rows.data(), rows.size() * sizeof(size_t), hipMemcpyHostToDevice));
        return HE_OK;
    }
    void release(void *with = nullptr) {  // the table, and what the set keeps beside it, once the stream is done with them
        if (!d_tab && !with) return;
        hipSetDevice(ev->be->ctx->dev);
        hipStreamSynchronize(ev->be->ctx->stream);
        hipFree(d_tab);
        hipFree(with);
    }
};
// BlindRotationEvaluationKeySet's keys: RGSW ciphertexts of one shape, each two key handles (table: rgsw0 | rgsw1)
struct RgswSet : KeySet {
    std::vector<std::shared_ptr<Evk>> k0, k1;
    RgswSet() : KeySet(T_RGSW_SET) {}
    ~RgswSet() override { release(); }
};
struct RgswShape {
    int levelQ = 0, levelP = -1;
    bool multiple_p = false;  // branch M (levelP >= 1): RNS digits; otherwise bit windows (pw2 == 0: one uncentred window per limb)
    bool fused = false;       // inside the domain of launch_rgsw_fused
    RgswShape() = default;
    explicit RgswShape(const Evk &k) : levelQ(k.nQk - 1), levelP(k.nPk - 1), multiple_p(levelP >= 1) {}  // the shape of a gadget key
};
// The window domain of the one-launch kernel: a standard ring, at most one special prime, the ring and level of
// rgsw_fused_supported, every window inside a 64-bit word and every window offset inside a byte.  launch_rgsw_fused serves all of
// it; launch_auto_fused its base-2 keys (pw2 != 0; hering_blindrot.h)
bool fused_window_domain(const BasisExtender &be, const Evk &k) {
    bool ok = be.type == 0 && k.nPk <= 1 && rgsw_fused_supported(be.Q->logN, k.nQk);
    for (int i = 0; ok && i < k.nQk; i++) ok = (rgsw_nj(k, i) - 1) * k.pw2 < 64 && (k.pw2 ? k.prefix[i] : i) < 256;
    return ok;
}
bool rgsw_same_shape(const Evk &a, const Evk &b) {
    return a.nQk == b.nQk && a.nPk == b.nPk && a.pw2 == b.pw2 && a.beta == b.beta && a.nj == b.nj;
}
int rgsw_shape(const char *who, const Evaluator &ev, const Evk &a, const Evk &b, RgswShape *s) {
    const BasisExtender &be = *ev.be;
    if (a.ev.get() != &ev || b.ev.get() != &ev) return fail(HE_EINVAL, "%s: key belongs to another evaluator", who);
    if (!rgsw_same_shape(a, b)) return fail(HE_EINVAL, "%s: the two gadget ciphertexts of an RGSW ciphertext differ in shape", who);
    *s = RgswShape(a);
    if (!a.pw2 && a.nPk == 0) return fail(HE_EINVAL, "%s: BaseTwoDecomposition == 0 needs a special prime", who);
    const int need = s->multiple_p ? base_rns_size(s->levelQ, s->levelP) : (a.pw2 ? a.prefix[s->levelQ + 1] : s->levelQ + 1);
    if (a.beta < need) return fail(HE_EINVAL, "%s: key has %d digits, %d needed", who, a.beta, need);
    // externalProduct32Bit (:84-128) sums plain 64-bit products key * NTTLazy(window) over both components' D windows, and
    // NTTLazy returns words up to 6q - 2 (ring/ntt.go:133): below 2^64 the sum is the value the bit-window branch computes,
    // at or above it the reference's output is an artefact of the wrap
    const uint64_t q0 = be.Q->moduli[0];
    if (s->levelQ == 0 && s->levelP == -1 && (q0 >> 29) == 0) {
        const u128 bound = (u128)2 * (u128)a.nj[0] * (u128)(6 * q0 - 2) * (u128)(q0 - 1);
        if ((bound >> 64) != 0)
            return fail(HE_EINVAL, "%s: 2 D W (q - 1) >= 2^64 (D = %d windows, W = 6q - 2, q = %llu): the 32-bit branch of the reference wraps",
                        who, a.nj[0], (unsigned long long)q0);
    }
    s->fused = fused_window_domain(be, a);
    return HE_OK;
}
// Key words at or above q (hering_rgsw.h, "Key words"): served where the reference's own arithmetic is exact with words below
// M q -- every MRed / MRedLazy(key, y) has key * y < q 2^64, y an NTTLazy word (at most 6q - 2) in the bit-window branch and a
// word below 2q in branch M; the 32-bit branch's plain sum stays below 2^64 -- and refused elsewhere.
int rgsw_key_words(const char *who, const Evaluator &ev, const Evk &a, const Evk &b, const RgswShape &s) {
    const uint64_t M = std::max(a.word_mul, b.word_mul);
    if (M <= 1) return HE_OK;  // (canonical keys: rgsw_shape has checked the 32-bit branch's bound)
    if (M >= Evk::kWordMulCap)
        return fail(HE_EINVAL, "%s: the key went through so many lazy helpers that no bound on its words is kept (HE_RGSW_REDUCE the key first)", who);
    const BasisExtender &be = *ev.be;
    const uint64_t q0 = be.Q->moduli[0];
    if (s.levelQ == 0 && s.levelP == -1 && (q0 >> 29) == 0) {
        const u128 bound = (u128)2 * (u128)a.nj[0] * (u128)(6 * q0 - 2) * (u128)(M * q0 - 1);  // M <= 2^32, q0 < 2^29
        if ((bound >> 64) != 0)
            return fail(HE_EINVAL, "%s: 2 D W (M q - 1) >= 2^64 with key words below M q, M = %llu (HE_RGSW_REDUCE the key first)",
                        who, (unsigned long long)M);
        return HE_OK;
    }
    for (int j = 0; j <= s.levelQ + s.levelP + 1; j++) {
        const uint64_t q = j <= s.levelQ ? be.Q->moduli[j] : be.P->moduli[j - s.levelQ - 1];
        const u128 kmax = (u128)M * q, ymax = s.multiple_p ? (u128)2 * q - 1 : (u128)6 * q - 2;
        if ((kmax >> 64) != 0 || (kmax - 1) * ymax >= ((u128)q << 64))
            return fail(HE_EINVAL, "%s: key words below M q, M = %llu, leave the domain of the reference's Montgomery products at q = %llu "
                        "(HE_RGSW_REDUCE the key first)", who, (unsigned long long)M, (unsigned long long)q);
    }
    return HE_OK;
}
// what both routes account for: two GadgetProductLazy, the sum of their accumulators and ModDown (or the copy)
void rgsw_account(Evaluator &ev, const Evk &k, const RgswShape &s, int B) {
    BasisExtender &be = *ev.be;
    const int nQ = s.levelQ + 1, nP = s.levelP + 1;
    const int beta = s.multiple_p ? base_rns_size(s.levelQ, s.levelP) : (k.pw2 ? k.prefix[nQ] : nQ);
    be.ctx->acct(4.0 * nQ, 2.0 * 2.0 * beta * (nQ + nP), B, be.Q->N);  // (in0, in1, out0, out1) and the rows of both keys
    Valu V(be.Q->logN);
    for (int c = 0; c < 2; c++) {
        if (s.multiple_p) valu_keyswitch(V, be, s.levelQ, s.levelP, beta, true, true);
        else {  // INTT of the component, one NTT and two products per (window, destination limb)
            for (int i = 0; i < nQ; i++) V.ntt(cls_f64(be.small, i));
            for (int j = 0; j < nQ + nP; j++) {
                const int m = j < nQ ? j : be.LQ + j - nQ;
                V.ntt(cls_f64(be.small, m), beta);
                V.mul(cls_f64(be.small, m), 2.0 * beta);
            }
        }
        if (nP > 0) valu_moddown(V, be, s.levelQ, s.levelP);
    }
    V.into(*be.ctx, B);
}
size_t rgsw_generic_words(const BasisExtender &be, const Evk &k, const RgswShape &s, int B) {
    const size_t N = be.Q->N, nQ = s.levelQ + 1, nP = s.levelP + 1;
    size_t beta = 0;
    if (s.multiple_p) beta = (size_t)base_rns_size(s.levelQ, s.levelP);
    else for (int i = 0; i <= s.levelQ; i++) beta += (size_t)rgsw_nj(k, i);
    const size_t one = (size_t)B * nQ * N + (size_t)B * beta * (be.LQ + be.LP) * N;  // INTT(in_k) and its digits
    return 2 * one + 2 * 2 * (size_t)B * (nQ + nP) * N + 2 * (size_t)B * (nQ + nP) * N + 256;
}
// the generic route: the accumulators of both components through the cores that exist, one sum, one ModDown over 2B entries
int rgsw_generic(Evaluator &ev, const Evk &ka, const Evk &kb, const RgswShape &s, View in0, View in1, View out0, View out1, int B) {
    BasisExtender &be = *ev.be;
    hipStream_t st = be.ctx->stream;
    const int levelQ = s.levelQ, levelP = s.levelP, N = be.Q->N;
    const size_t sQw = (size_t)(levelQ + 1) * N, sPw = (size_t)(levelP + 1) * N, W = sQw + sPw;
    TRY(be.ctx->arena_reserve(rgsw_generic_words(be, ka, s, B)));
    // acc[k]: [2 output components][B] entries of Q limbs then P limbs, so that one launch covers both rings and components
    uint64_t *acc[2] = {be.ctx->arena_take(2 * (size_t)B * W), be.ctx->arena_take(2 * (size_t)B * W)};
    const View none{nullptr, 0};
    for (int k = 0; k < 2; k++) {
        const Evk &key = k ? kb : ka;
        const View cx = k ? in1 : in0;
        const View o0Q{acc[k], W}, o1Q{acc[k] + (size_t)B * W, W};
        const View o0P = levelP < 0 ? none : View{acc[k] + sQw, W}, o1P = levelP < 0 ? none : View{acc[k] + (size_t)B * W + sQw, W};
        const LazyArgs a{cx, B, o0Q, o0P, o1Q, o1P};
        KsCall c;
        if (s.multiple_p) {  // (RNS digits; a base-2 gadget takes at most one special prime, he_evk_create_base2)
            TRY(ks_call(ev, KS_LAZY, levelQ, key, KsAlias{}, &c));
            TRY(gadget_product_lazy_core(ev, levelQ, key, c, a));
        } else TRY(window_products_core(ev, levelQ, key, a, true));
    }
    if (levelP < 0) {  // ModDown's levelP == -1 branch is a copy: the sum goes straight to the outputs
        const LimbTab tq = ident_tab(levelQ + 1);
        HIP_TRY(launch_ew(be.qp, tq, EW_ADD, View{acc[0], W}, View{acc[1], W}, out0, B, nullptr, nullptr, st));
        HIP_TRY(launch_ew(be.qp, tq, EW_ADD, View{acc[0] + (size_t)B * W, W}, View{acc[1] + (size_t)B * W, W}, out1, B, nullptr, nullptr, st));
        return HE_OK;
    }
    LimbTab t;
    t.n = 0;
    for (int j = 0; j <= levelQ; j++, t.n++) { t.in_limb[t.n] = t.out_limb[t.n] = (uint8_t)t.n; t.mod[t.n] = (uint8_t)j; }
    for (int j = 0; j <= levelP; j++, t.n++) { t.in_limb[t.n] = t.out_limb[t.n] = (uint8_t)t.n; t.mod[t.n] = (uint8_t)(be.LQ + j); }
    HIP_TRY(launch_ew(be.qp, t, EW_ADD, View{acc[0], W}, View{acc[1], W}, View{acc[0], W}, 2 * B, nullptr, nullptr, st));
    View sP{be.ctx->arena_take(2 * (size_t)B * sPw), sPw}, sQ{be.ctx->arena_take(2 * (size_t)B * sQw), sQw};
    TRY(moddown_front(ev, levelQ, levelP, View{acc[0] + sQw, W}, sP, sQ, 2 * B, true));
    TRY(moddown_back(ev, levelQ, levelP, sQ, View{acc[0], W}, out0, nullptr, B));
    TRY(moddown_back(ev, levelQ, levelP, View{sQ.p + (size_t)B * sQw, sQw}, View{acc[0] + (size_t)B * W, W}, out1, nullptr, B));
    return HE_OK;
}
// the fused route's arguments for keys of shape k (key0 / key1 / ktab are the caller's)
void rgsw_fused_args(RgswFusedArgs &a, const BasisExtender &be, const Evk &k, const RgswShape &s, View in0, View in1, View out0, View out1) {
    a.in0 = in0; a.in1 = in1; a.out0 = out0; a.out1 = out1;
    a.nQ = s.levelQ + 1; a.nP = s.levelP + 1; a.p_mod = be.LQ;
    a.key_limbs = k.nQk + k.nPk; a.key_p_limb = k.nQk;
    a.pw2 = k.pw2;
    a.mask = k.pw2 ? ((uint64_t)1 << k.pw2) - 1 : ~(uint64_t)0;
    const uint64_t p = a.nP ? be.P->moduli[0] : 0;
    a.p_half = a.nP ? (p - 1) / 2 : 0;
    for (int i = 0; i < kRgswMaxQ; i++) { a.nj[i] = a.prefix[i] = 0; a.md_s[i] = a.p_mod_q[i] = 0; }
    for (int i = 0; i < a.nQ; i++) {
        a.nj[i] = (uint8_t)rgsw_nj(k, i);
        a.prefix[i] = (uint8_t)(k.pw2 ? k.prefix[i] : i);
        if (a.nP) { a.md_s[i] = be.Q->moduli[i] - be.md_ptoq[0][i]; a.p_mod_q[i] = p % be.Q->moduli[i]; }
    }
}
// operands shared by the two product entries: (in0, in1, out0, out1), out_k == in_k allowed
int rgsw_operands(Operands &o, int nQ, he_handle in0, he_handle in1, he_handle out0, he_handle out1) {
    const int i0 = o.in(in0, nQ, "in0"), i1 = o.in(in1, nQ, "in1");
    const int o0 = o.out(out0, nQ, "out0"), o1 = o.out(out1, nQ, "out1");
    o.inplace(o0, i0);
    o.inplace(o1, i1);
    return o.check();
}
// What he_rgsw_external_product_select and he_automorphism_ct_select share before their request is filed.  `shape` is the entry's
// own check of its keys' shape, digits and one-launch domain (it fills *s); then the key words of every key (k1: the second
// gadget ciphertext of key i, or k0 again), the selection, the operands, the request's blob and the frozen copy of the selection.
int select_request(const char *who, const std::shared_ptr<Evaluator> &ev, const std::shared_ptr<KeySet> &set,
                   const std::vector<std::shared_ptr<Evk>> &k0, const std::vector<std::shared_ptr<Evk>> &k1,
                   const std::function<int(RgswShape *)> &shape, const int32_t *sel, int n_sel, he_handle in0, he_handle in1,
                   he_handle out0, he_handle out1, RgswShape *s, CoReq &q, std::vector<int32_t> *selv) {
    if (set->ev.get() != ev.get()) return fail(HE_EINVAL, "%s: key set belongs to another evaluator", who);
    TRY(shape(s));
    for (size_t i = 0; i < k0.size(); i++) TRY(rgsw_key_words(who, *ev, *k0[i], *k1[i], *s));
    if (!sel || n_sel < 1) return fail(HE_EINVAL, "%s: null selection", who);
    const int n = (int)k0.size();
    for (int b = 0; b < n_sel; b++)
        if (sel[b] < -1 || sel[b] >= n) return fail(HE_EINVAL, "%s: sel[%d] = %d outside [-1, %d)", who, b, (int)sel[b], n);
    Operands o(q, who, *ev->be);
    TRY(rgsw_operands(o, s->levelQ + 1, in0, in1, out0, out1));
    if (n_sel != o.B) return fail(HE_EINVAL, "%s: n_sel = %d, the batch has %d entries", who, n_sel, o.B);
    q.obj = ev.get(); q.key = set.get();
    for (int b = 0; b < n_sel; b++) q.blob.push_back((uint64_t)(int64_t)sel[b]);
    q.keep.push_back(ev); q.keep.push_back(set);
    selv->assign(sel, sel + n_sel);  // frozen here: a scalar argument of the call
    return HE_OK;
}
// ... and when it runs (`account(used)` and `launch` are the entry's own): the selection into scratch, the set's resident table
int select_run(const char *who, const KeySet &set, const std::vector<std::shared_ptr<Evk>> &k0, const RgswShape &s, const std::vector<int32_t> &selv,
               const View *v, int B, const std::function<void(int)> &account, decltype(launch_rgsw_fused) *launch) {
    BasisExtender &be = *set.ev->be;
    if ((int)selv.size() != B) return fail(HE_EINVAL, "%s: selection of %d for %d entries", who, (int)selv.size(), B);
    account((int)std::count_if(selv.begin(), selv.end(), [](int32_t x) { return x >= 0; }));
    RgswFusedArgs a;
    rgsw_fused_args(a, be, *k0[0], s, v[0], v[1], v[2], v[3]);
    a.ktab = set.d_tab; a.nkeys = (int)k0.size();
    TRY(scratch_selection(*be.ctx, selv.data(), selv.size(), &a.sel));
    HIP_TRY(launch(be.qp, a, B, be.ctx->stream));
    return HE_OK;
}
}  // namespace

namespace {
bool rgsw_no_fused() {
    static const bool v = env_flag("HERING_NO_RGSW_FUSED");
    return v;
}
// the launches of he_rgsw_external_product over B entries (s.fused: the one-launch kernel); the caller holds the context
int rgsw_product_run(Evaluator &ev, const Evk &k0, const Evk &k1, const RgswShape &s, const View *v, int B) {
    BasisExtender &be = *ev.be;
    rgsw_account(ev, k0, s, B);
    if (!s.fused) {
        // both components of the batch go in one launch, 2 B entries along the grid's z: chunks of at most 32767 entries
        for (int b0 = 0; b0 < B; b0 += 32767) {
            View c[4];
            for (int i = 0; i < 4; i++) c[i] = View{v[i].p + (size_t)b0 * v[i].bstride, v[i].bstride};
            be.ctx->arena_reset();
            TRY(rgsw_generic(ev, k0, k1, s, c[0], c[1], c[2], c[3], std::min(32767, B - b0)));
        }
        return HE_OK;
    }
    RgswFusedArgs a;
    rgsw_fused_args(a, be, k0, s, v[0], v[1], v[2], v[3]);
    a.key0 = k0.d; a.key1 = k1.d;
    HIP_TRY(launch_rgsw_fused(be.qp, a, B, be.ctx->stream));
    return HE_OK;
}
}  // namespace

int he_rgsw_external_product(he_handle hev, he_handle in0, he_handle in1, he_handle hk0, he_handle hk1, he_handle out0, he_handle out1) {
    static const char *who = "he_rgsw_external_product";
    GET(ev, Evaluator, hev, T_EVAL);
    GET(k0, Evk, hk0, T_EVK);
    GET(k1, Evk, hk1, T_EVK);
    BasisExtender &be = *ev->be;
    RgswShape s;
    TRY(rgsw_shape(who, *ev, *k0, *k1, &s));
    TRY(rgsw_key_words(who, *ev, *k0, *k1, s));
    if (rgsw_no_fused()) s.fused = false;
    CoReq q;
    Operands o(q, who, be);
    TRY(rgsw_operands(o, s.levelQ + 1, in0, in1, out0, out1));
    q.op = CO_RGSW; q.obj = ev.get(); q.key = k0.get(); q.par[0] = (int64_t)(uintptr_t)k1.get(); q.par[1] = 0;
    q.keep.push_back(ev); q.keep.push_back(k0); q.keep.push_back(k1);
    q.run = [ev, k0, k1, s](const View *v, int B) -> int { return rgsw_product_run(*ev, *k0, *k1, s, v, B); };
    q.one_by_one();  // (queued calls are served one by one, as other base-2 shapes)
    return co_dispatch(*be.ctx, o.B, q);
}
int he_rgsw_keyset_create(he_handle hev, int n, const he_handle *rgsw0, const he_handle *rgsw1, he_handle *out) {
    static const char *who = "he_rgsw_keyset_create";
    GET(ev, Evaluator, hev, T_EVAL);
    if (n < 1 || !rgsw0 || !rgsw1 || !out) return fail(HE_EINVAL, "%s: at least one RGSW ciphertext and an output are needed", who);
    auto set = std::make_shared<RgswSet>();
    set->ev = ev;
    for (int i = 0; i < n; i++) {
        std::shared_ptr<Evk> a = get<Evk>(rgsw0[i], T_EVK), b = get<Evk>(rgsw1[i], T_EVK);
        if (!a || !b) return fail(HE_EHANDLE, "%s: bad Evk handle (key %d)", who, i);
        RgswShape s;
        TRY(rgsw_shape(who, *ev, *a, *b, &s));
        if (i > 0 && !rgsw_same_shape(*a, *set->k0[0])) return fail(HE_EINVAL, "%s: key %d differs in shape from key 0", who, i);
        set->k0.push_back(a); set->k1.push_back(b);
    }
    std::vector<size_t> tab(2 * (size_t)n);
    for (int i = 0; i < n; i++) { tab[i] = (size_t)(uintptr_t)set->k0[i]->d; tab[(size_t)n + i] = (size_t)(uintptr_t)set->k1[i]->d; }
    Scope sc(ev->be->ctx.get());
    TRY(set->upload(tab));
    *out = reg(set);
    return HE_OK;
}
int he_rgsw_keyset_destroy(he_handle h) { return unreg(h, T_RGSW_SET); }
int he_rgsw_external_product_select(he_handle hev, he_handle in0, he_handle in1, he_handle hset, const int32_t *sel, int n_sel,
                                    he_handle out0, he_handle out1) {
    static const char *who = "he_rgsw_external_product_select";
    GET(ev, Evaluator, hev, T_EVAL);
    GET(set, RgswSet, hset, T_RGSW_SET);
    RgswShape s;
    CoReq q;
    std::vector<int32_t> selv;
    auto shape = [&](RgswShape *sh) -> int {
        TRY(rgsw_shape(who, *ev, *set->k0[0], *set->k1[0], sh));
        if (!sh->fused) return fail(HE_EINVAL, "%s: the shape is outside the domain of the one-launch kernel (hering_rgsw.h)", who);
        return HE_OK;
    };
    TRY(select_request(who, ev, set, set->k0, set->k1, shape, sel, n_sel, in0, in1, out0, out1, &s, q, &selv));
    q.op = CO_RGSW; q.par[1] = 1;
    q.run = [ev, set, s, selv](const View *v, int B) -> int {
        auto account = [&](int used) {
            if (used) rgsw_account(*ev, *set->k0[0], s, used);
            ev->be->ctx->acct(4.0 * (s.levelQ + 1), 0, B - used, ev->be->Q->N);
        };
        return select_run(who, *set, set->k0, s, selv, v, B, account, launch_rgsw_fused);
    };
    q.one_by_one();
    return co_dispatch(*ev->be->ctx, (int)selv.size(), q);
}

// ---- the element-wise helpers of core/rgsw/evaluator.go:283-356 on the words of a device-resident gadget ciphertext ----------
namespace {
// one element-wise launch over the Q limbs of every row and one over the P limbs (y: a polynomial of the Q / P ring shared by the
// rows, or the rows of another key when yQ.p is null)
int key_rows_ew(const Evk &out, int op, View x, View yQ, View yP, View ykey) {
    BasisExtender &be = *out.ev->be;
    const int nQ = out.nQk, nP = out.nPk, rows = 2 * out.beta;
    hipStream_t st = be.ctx->stream;
    const View z = out.rows();
    if (!yQ.p) {  // key (op) key: one launch over all limbs
        LimbTab t;
        t.n = 0;
        for (int j = 0; j < nQ + nP; j++, t.n++) { t.in_limb[t.n] = t.out_limb[t.n] = (uint8_t)j; t.mod[t.n] = (uint8_t)(j < nQ ? j : be.LQ + j - nQ); }
        HIP_TRY(launch_ew(be.qp, t, op, x, ykey, z, rows, nullptr, nullptr, st));
        return HE_OK;
    }
    HIP_TRY(launch_ew(be.qp, ident_tab(nQ), op, x, yQ, z, rows, nullptr, nullptr, st));
    if (nP > 0) {
        LimbTab t;
        uint8_t xl[kMaxLimbs];
        t.n = nP;
        for (int j = 0; j < nP; j++) { t.in_limb[j] = (uint8_t)j; t.out_limb[j] = xl[j] = (uint8_t)(nQ + j); t.mod[j] = (uint8_t)(be.LQ + j); }
        HIP_TRY(launch_ew(be.qp, t, op, x, yP, z, rows, nullptr, xl, st));
    }
    return HE_OK;
}
}  // namespace
int he_rgsw_key_op(int op, he_handle hin, he_handle hxQ, he_handle hxP, he_handle hout) {
    static const char *who = "he_rgsw_key_op";
    GET(in, Evk, hin, T_EVK);
    GET(out, Evk, hout, T_EVK);
    if (in->ev.get() != out->ev.get() || !rgsw_same_shape(*in, *out)) return fail(HE_EINVAL, "%s: the two keys differ in evaluator or shape", who);
    BasisExtender &be = *out->ev->be;
    const bool mul = op == HE_RGSW_MUL_LAZY || op == HE_RGSW_MUL_THEN_ADD_LAZY;
    if (!mul && op != HE_RGSW_ADD_LAZY && op != HE_RGSW_REDUCE) return fail(HE_EINVAL, "%s: unknown operation %d", who, op);
    std::shared_ptr<Poly> xQ, xP;
    if (mul) {
        xQ = get<Poly>(hxQ, T_POLY);
        if (out->nPk > 0) xP = get<Poly>(hxP, T_POLY);
        if (!xQ || (out->nPk > 0 && !xP)) return fail(HE_EHANDLE, "%s: bad Poly handle for powXMinusOne", who);
        for (const Poly *x : {xQ.get(), xP.get()}) {
            if (!x) continue;
            if (x->ctx != be.ctx || x->N != be.Q->N || x->batch != 1 || x->nlimbs < (x == xQ.get() ? out->nQk : out->nPk))
                return fail(HE_EINVAL, "%s: powXMinusOne is one polynomial of the evaluator's degree with the key's limbs", who);
        }
    }
    Scope sc(be.ctx.get());
    const int rows = 2 * out->beta, limbs = out->nQk + out->nPk;
    be.ctx->acct((op == HE_RGSW_REDUCE ? 2.0 : 3.0) * limbs, mul ? limbs : 0, rows, be.Q->N);
    if (mul) { Valu V(be.Q->logN); for (int j = 0; j < limbs; j++) V.mul(cls_f64(be.small, j < out->nQk ? j : be.LQ + j - out->nQk), 1.0); V.into(*be.ctx, rows); }
    const View none{nullptr, 0};
    const uint64_t add = op == HE_RGSW_ADD_LAZY ? in->word_mul : 2;  // (MRedLazy returns words below 2q)
    const uint64_t mul_after = op == HE_RGSW_REDUCE ? 1 : std::min(Evk::kWordMulCap, (op == HE_RGSW_MUL_LAZY ? 0 : out->word_mul) + add);
    if (op != HE_RGSW_REDUCE) out->word_mul = std::max(out->word_mul, mul_after);  // (a launch that fails may have written some rows)
    switch (op) {
        case HE_RGSW_ADD_LAZY: TRY(key_rows_ew(*out, EW_ADD_LAZY, out->rows(), none, none, in->rows())); break;
        case HE_RGSW_REDUCE: TRY(key_rows_ew(*out, EW_REDUCE, in->rows(), none, none, in->rows())); break;
        default:
            TRY(key_rows_ew(*out, op == HE_RGSW_MUL_LAZY ? EW_MUL_MONT_LAZY : EW_MUL_MONT_LAZY_THEN_ADD_LAZY, in->rows(),
                            View{xQ->d, 0}, xP ? View{xP->d, 0} : none, none));
    }
    out->word_mul = mul_after;  // (Reduce lowers the bound only once its launch has been made)
    return evk_derive(*out);  // (he_evk_commit's launches, in stream order)
}
int he_rgsw_key_add_plaintext_lazy(he_handle hpt, he_handle hk0, he_handle hk1) {
    static const char *who = "he_rgsw_key_add_plaintext_lazy";
    GET(pt, Poly, hpt, T_POLY);
    GET(k0, Evk, hk0, T_EVK);
    GET(k1, Evk, hk1, T_EVK);
    if (k0->ev.get() != k1->ev.get() || !rgsw_same_shape(*k0, *k1) || k0.get() == k1.get())
        return fail(HE_EINVAL, "%s: the two gadget ciphertexts of an RGSW ciphertext are distinct keys of one evaluator and shape", who);
    BasisExtender &be = *k0->ev->be;
    const int nQ = k0->nQk, N = be.Q->N;
    const int nP = k0->nPk > 0 ? k0->nPk : 1;  // (:290-292)
    int maxj = 1;
    for (int i = 0; k0->pw2 && i < nQ; i++) maxj = std::max(maxj, k0->nj[i]);
    if (pt->ctx != be.ctx || pt->N != N || pt->nlimbs < nQ || pt->batch < maxj)
        return fail(HE_EINVAL, "%s: the plaintext holds one polynomial of %d limbs per window (%d windows)", who, nQ, maxj);
    const int digits = k0->pw2 ? nQ : k0->beta;
    // (polynomial words lie in [0, 2q); raised before the launches: one that fails may have written some rows)
    for (Evk *k : {k0.get(), k1.get()}) k->word_mul = std::min(Evk::kWordMulCap, k->word_mul + 2);
    Scope sc(be.ctx.get());
    hipStream_t st = be.ctx->stream;
    const size_t rs = (size_t)(k0->nQk + k0->nPk) * N;
    int d = 0;
    for (int i = 0; i < digits; i++) {
        const int start = i * nP, end = std::min((i + 1) * nP, nQ);
        const int wj = k0->pw2 ? k0->nj[i] : 1;
        for (int j = 0; j < wj; j++, d++) {
            if (start >= end) continue;
            const LimbTab t = ident_tab(end - start, start, start, start);
            const View y{pt->d + (size_t)j * pt->nlimbs * N, 0};
            for (int c = 0; c < 2; c++) {  // Value[0][i][j][0] and Value[1][i][j][1]
                const View row{(c ? k1->d : k0->d) + ((size_t)d * 2 + c) * rs, 0};
                HIP_TRY(launch_ew(be.qp, t, EW_ADD_LAZY, row, y, row, 1, nullptr, nullptr, st));
            }
            be.ctx->acct(6.0 * (end - start), 0, 1, N);
        }
    }
    TRY(evk_derive(*k0));
    return evk_derive(*k1);
}

// ---------------------------------------------------------------------------------------
// Blind rotation (include/hering_blindrot.h; core/rgsw/blindrot/evaluator.go)
// ---------------------------------------------------------------------------------------
namespace {
// BlindRotationEvaluationKeySet's automorphism keys: Galois keys of one shape with their Galois elements
// (table: the keys' words | their index tables)
struct GaloisSet : KeySet {
    std::vector<std::shared_ptr<Evk>> keys;
    std::vector<uint64_t> gal;
    uint32_t *d_index = nullptr;  // [n][N] AutomorphismNTTWithIndex tables
    GaloisSet() : KeySet(T_GALOIS_SET) {}
    ~GaloisSet() override { release(d_index); }
    int find(uint64_t g) const {
        for (size_t i = 0; i < gal.size(); i++)
            if (gal[i] == g) return (int)i;
        return -1;
    }
};
// the bytes and arithmetic of `used` automorphisms with keys of shape k and of B - used copies
void auto_select_account(Evaluator &ev, const Evk &k, int used, int B) {
    BasisExtender &be = *ev.be;
    const int level = k.nQk - 1;
    if (used) {
        be.ctx->acct(4.0 * (level + 1) + key_limbs(k, level), 0, used, be.Q->N);  // (every entry reads its own key)
        Valu V(be.Q->logN);
        valu_gadget_product(V, be, level, k.nPk - 1, key_beta(k, level), true);
        V.into(*be.ctx, used);
    }
    be.ctx->acct(4.0 * (level + 1), 0, B - used, be.Q->N);
}
// what he_blind_rotate_core decided on the host before it filed its request
struct BlindrotPlan {
    std::vector<std::vector<blindrot::Op>> lists;  // per entry (every Galois element has a key in the set)
    // the batched route: [rounds][2][B] selections (automorphism | external product) and which launches have something to do
    std::vector<int32_t> sel;
    std::vector<uint8_t> any;  // [rounds][2]
    size_t n_auto = 0, n_prod = 0;
};
int blindrot_batched(Evaluator &ev, const RgswSet &rset, const GaloisSet &gset, const RgswShape &s, const BlindrotPlan &p, View acc0,
                     View acc1, int B) {
    BasisExtender &be = *ev.be;
    hipStream_t st = be.ctx->stream;
    const int32_t *dsel = nullptr;  // the selections of every round (as the select forms do)
    TRY(scratch_selection(*be.ctx, p.sel.data(), p.sel.size(), &dsel));
    const Evk &gk = *gset.keys[0];
    RgswFusedArgs ap, aa;
    rgsw_fused_args(ap, be, *rset.k0[0], s, acc0, acc1, acc0, acc1);
    ap.ktab = rset.d_tab; ap.nkeys = (int)rset.k0.size();
    rgsw_fused_args(aa, be, gk, RgswShape(gk), acc0, acc1, acc0, acc1);
    aa.ktab = gset.d_tab; aa.nkeys = (int)gset.keys.size();
    if (p.n_prod) rgsw_account(ev, *rset.k0[0], s, (int)p.n_prod);
    auto_select_account(ev, gk, (int)p.n_auto, (int)p.n_auto);
    const size_t rounds = p.any.size() / 2;
    for (size_t r = 0; r < rounds; r++) {
        if (p.any[2 * r]) {
            aa.sel = dsel + (2 * r) * (size_t)B;
            HIP_TRY(launch_auto_fused(be.qp, aa, B, st));
        }
        if (p.any[2 * r + 1]) {
            ap.sel = dsel + (2 * r + 1) * (size_t)B;
            HIP_TRY(launch_rgsw_fused(be.qp, ap, B, st));
        }
    }
    return HE_OK;
}
// the reference's own order, entry by entry, through the launches of he_rgsw_external_product and he_automorphism_ct
int blindrot_per_entry(Evaluator &ev, const RgswSet &rset, const GaloisSet &gset, RgswShape s, const BlindrotPlan &p, View acc0,
                       View acc1, int B) {
    BasisExtender &be = *ev.be;
    if (rgsw_no_fused()) s.fused = false;
    for (int b = 0; b < B; b++) {
        const View c0{acc0.p + (size_t)b * acc0.bstride, acc0.bstride}, c1{acc1.p + (size_t)b * acc1.bstride, acc1.bstride};
        const View v[4] = {c0, c1, c0, c1};
        for (const blindrot::Op &op : p.lists[(size_t)b]) {
            be.ctx->arena_reset();  // (stream order: the previous operation's scratch is free once this one's launches run)
            if (op.kind == blindrot::OP_EXTERNAL_PRODUCT) TRY(rgsw_product_run(ev, *rset.k0[op.arg], *rset.k1[op.arg], s, v, 1));
            else TRY(automorphism_core(ev, s.levelQ, c0, &c1, nullptr, op.arg, *gset.keys[(size_t)gset.find(op.arg)], c0, c1, 1, KsAlias{true, true, false}));
        }
    }
    return HE_OK;
}
}  // namespace

int he_galois_keyset_create(he_handle hev, int n, const uint64_t *gal_els, const he_handle *keys, he_handle *out) {
    static const char *who = "he_galois_keyset_create";
    GET(ev, Evaluator, hev, T_EVAL);
    if (n < 1 || !gal_els || !keys || !out) return fail(HE_EINVAL, "%s: at least one Galois key, its element and an output are needed", who);
    const BasisExtender &be = *ev->be;
    auto set = std::make_shared<GaloisSet>();
    set->ev = ev;
    for (int i = 0; i < n; i++) {
        std::shared_ptr<Evk> k = get<Evk>(keys[i], T_EVK);
        if (!k) return fail(HE_EHANDLE, "%s: bad Evk handle (key %d)", who, i);
        if (k->ev.get() != ev.get()) return fail(HE_EINVAL, "%s: key %d belongs to another evaluator", who, i);
        if (i > 0 && !rgsw_same_shape(*k, *set->keys[0])) return fail(HE_EINVAL, "%s: key %d differs in shape from key 0", who, i);
        if (!(gal_els[i] & 1)) return fail(HE_EINVAL, "%s: Galois element %d must be odd", who, i);
        const uint64_t g = reduce_gal(gal_els[i], be.Q->logN, be.type);
        if (set->find(g) >= 0) return fail(HE_EINVAL, "%s: Galois element %llu is listed twice", who, (unsigned long long)g);
        set->keys.push_back(k); set->gal.push_back(g);
    }
    const size_t N = be.Q->N;
    Scope sc(be.ctx.get());
    HIP_TRY(hipMalloc((void **)&set->d_index, (size_t)n * N * sizeof(uint32_t)));
    std::vector<size_t> tab(2 * (size_t)n);
    for (int i = 0; i < n; i++) {
        uint32_t *ix = set->d_index + (size_t)i * N;
        HIP_TRY(launch_build_automorphism_index(be.Q->logN, be.Q->logN + be.type, set->gal[i], ix, be.ctx->stream));
        tab[i] = (size_t)(uintptr_t)set->keys[i]->d; tab[(size_t)n + i] = (size_t)(uintptr_t)ix;
    }
    TRY(set->upload(tab));
    HIP_TRY(hipStreamSynchronize(be.ctx->stream));
    *out = reg(set);
    return HE_OK;
}
int he_galois_keyset_destroy(he_handle h) { return unreg(h, T_GALOIS_SET); }
int he_automorphism_ct_select(he_handle hev, he_handle in0, he_handle in1, he_handle hset, const int32_t *sel, int n_sel,
                              he_handle out0, he_handle out1) {
    static const char *who = "he_automorphism_ct_select";
    GET(ev, Evaluator, hev, T_EVAL);
    GET(set, GaloisSet, hset, T_GALOIS_SET);
    RgswShape s;
    CoReq q;
    std::vector<int32_t> selv;
    auto shape = [&](RgswShape *sh) -> int {
        const Evk &k = *set->keys[0];
        if (!k.pw2 || !fused_window_domain(*ev->be, k)) return fail(HE_EINVAL, "%s: the shape is outside the domain of the one-launch kernel (hering_blindrot.h)", who);
        if (k.beta < k.prefix[k.nQk]) return fail(HE_EINVAL, "%s: key has %d digits, %d needed", who, k.beta, k.prefix[k.nQk]);
        *sh = RgswShape(k);
        return HE_OK;
    };
    TRY(select_request(who, ev, set, set->keys, set->keys, shape, sel, n_sel, in0, in1, out0, out1, &s, q, &selv));
    q.op = CO_AUTO_SELECT;
    q.run = [ev, set, s, selv](const View *v, int B) -> int {
        auto account = [&](int used) { auto_select_account(*ev, *set->keys[0], used, B); };
        return select_run(who, *set, set->keys, s, selv, v, B, account, launch_auto_fused);
    };
    q.one_by_one();
    return co_dispatch(*ev->be->ctx, (int)selv.size(), q);
}
int he_blind_rotate_core(he_handle hev, const uint64_t *a, int batch, int n_lwe, he_handle acc0, he_handle acc1, he_handle hrset,
                         he_handle hgset) {
    static const char *who = "he_blind_rotate_core";
    GET(ev, Evaluator, hev, T_EVAL);
    GET(rset, RgswSet, hrset, T_RGSW_SET);
    GET(gset, GaloisSet, hgset, T_GALOIS_SET);
    BasisExtender &be = *ev->be;
    if (rset->ev.get() != ev.get() || gset->ev.get() != ev.get()) return fail(HE_EINVAL, "%s: key set belongs to another evaluator", who);
    if (!a || batch < 1 || n_lwe < 1) return fail(HE_EINVAL, "%s: null or empty rows", who);
    if ((size_t)n_lwe > rset->k0.size()) return fail(HE_EINVAL, "%s: rows of %d words, the RGSW set has %d keys", who, n_lwe, (int)rset->k0.size());
    RgswShape s;
    TRY(rgsw_shape(who, *ev, *rset->k0[0], *rset->k1[0], &s));
    for (int i = 0; i < n_lwe; i++) TRY(rgsw_key_words(who, *ev, *rset->k0[i], *rset->k1[i], s));
    const Evk &gk = *gset->keys[0];
    if (gk.nQk - 1 != s.levelQ) return fail(HE_EINVAL, "%s: the Galois keys have level %d, the RGSW keys level %d", who, gk.nQk - 1, s.levelQ);
    CoReq q;
    Operands o(q, who, be);
    o.out(acc0, s.levelQ + 1, "acc0");
    o.out(acc1, s.levelQ + 1, "acc1");
    TRY(o.check());
    if (batch != o.B) return fail(HE_EINVAL, "%s: %d rows, the accumulator has %d entries", who, batch, o.B);
    const int B = o.B, logN = be.Q->logN;
    auto plan = std::make_shared<BlindrotPlan>();
    plan->lists.resize((size_t)B);
    for (int b = 0; b < B; b++) {
        if (!blindrot::blindrot_ops(logN, a + (size_t)b * n_lwe, n_lwe, &plan->lists[(size_t)b]))
            return fail(HE_EINVAL, "%s: row %d holds a word that is even and not zero, or not below 2N: no element of Z_2N^*", who, b);
        for (blindrot::Op &op : plan->lists[(size_t)b]) {
            if (op.kind != blindrot::OP_AUTOMORPHISM) continue;
            if (gset->find(op.arg) < 0) return fail(HE_EINVAL, "%s: the Galois set has no key for the element %llu", who, (unsigned long long)op.arg);
        }
    }
    static const bool no_batch = env_flag("HERING_NO_BLINDROT_BATCH");
    const bool batched = !no_batch && !rgsw_no_fused() && s.fused && gk.pw2 && fused_window_domain(be, gk) && gk.beta >= gk.prefix[gk.nQk];
    if (batched) {
        for (size_t i = 0; i < gset->keys.size(); i++) TRY(rgsw_key_words(who, *ev, *gset->keys[i], *gset->keys[i], RgswShape(gk)));
        const std::vector<blindrot::Round> rounds = blindrot::blindrot_merge(plan->lists);
        plan->sel.assign(rounds.size() * 2 * (size_t)B, -1);
        plan->any.assign(rounds.size() * 2, 0);
        for (size_t r = 0; r < rounds.size(); r++)
            for (int b = 0; b < B; b++) {
                const uint64_t g = rounds[r].gal[(size_t)b];
                const int32_t p = rounds[r].prod[(size_t)b];
                if (g) { plan->sel[(2 * r) * (size_t)B + b] = gset->find(g); plan->any[2 * r] = 1; plan->n_auto++; }
                if (p >= 0) { plan->sel[(2 * r + 1) * (size_t)B + b] = p; plan->any[2 * r + 1] = 1; plan->n_prod++; }
            }
    } else {
        for (int i = 0; i < (int)gset->keys.size(); i++) {
            int level = s.levelQ;
            TRY(check_key(*ev, *gset->keys[i], level, who));
        }
    }
    q.op = CO_BLINDROT; q.obj = ev.get(); q.key = rset.get(); q.par[0] = (int64_t)(uintptr_t)gset.get(); q.par[1] = n_lwe;
    q.blob.assign(a, a + (size_t)B * n_lwe);
    q.keep.push_back(ev); q.keep.push_back(rset); q.keep.push_back(gset);
    q.run = [ev, rset, gset, s, plan, batched](const View *v, int B) -> int {
        if ((int)plan->lists.size() != B) return fail(HE_EINVAL, "he_blind_rotate_core: %d rows for %d entries", (int)plan->lists.size(), B);
        return batched ? blindrot_batched(*ev, *rset, *gset, s, *plan, v[0], v[1], B)
                       : blindrot_per_entry(*ev, *rset, *gset, s, *plan, v[0], v[1], B);
    };
    q.one_by_one();
    return co_dispatch(*be.ctx, o.B, q);
}

// ---------------------------------------------------------------------------------------
// lintrans.Evaluator (include/hering_lintrans.h; circuits/common/lintrans): the index on the host, the LinearTransformation
// handle, and EvaluateMany as one request composed of the launches of he_decompose_ntt, he_automorphism_hoisted_lazy, the
// grouped multiply-accumulate kernel, he_eval_moddown_qp_to_q_ntt and he_lintrans_giant_step
// ---------------------------------------------------------------------------------------
int he_lintrans_bsgs_index(const int *diag, int n, int slots, int N1, int *rotN1, int *n1, int *rotN2, int *n2, int *index) {
    static const char *who = "he_lintrans_bsgs_index";
    if (n < 0 || (n > 0 && !diag) || !n1 || !n2) return fail(HE_EINVAL, "%s: null argument", who);
    if (slots < 1 || (slots & (slots - 1)) || N1 < 1 || (N1 & (N1 - 1))) return fail(HE_EINVAL, "%s: slots and N1 must be powers of two", who);
    const lintrans::BsgsIndex ix = lintrans::bsgs_index(diag, n, slots, N1);
    if (rotN1) std::copy(ix.rotN1.begin(), ix.rotN1.end(), rotN1);
    if (rotN2) std::copy(ix.rotN2.begin(), ix.rotN2.end(), rotN2);
    *n1 = (int)ix.rotN1.size(); *n2 = (int)ix.rotN2.size();
    if (index)
        for (int k = 0; k < n; k++) {
            const int64_t rot = (int64_t)diag[k] & ((int64_t)slots - 1);
            index[2 * k] = (int)(((rot / N1) * N1) & ((int64_t)slots - 1));
            index[2 * k + 1] = (int)(rot & ((int64_t)N1 - 1));
        }
    return HE_OK;
}
int he_lintrans_find_best_bsgs_ratio(const int *diag, int n, int maxN, int logMaxRatio, int *N1) {
    static const char *who = "he_lintrans_find_best_bsgs_ratio";
    if (n < 0 || (n > 0 && !diag) || !N1) return fail(HE_EINVAL, "%s: null argument", who);
    if (maxN < 1 || (maxN & (maxN - 1)) || logMaxRatio < 0 || logMaxRatio > 30) return fail(HE_EINVAL, "%s: maxN must be a power of two and logMaxRatio in [0, 30]", who);
    *N1 = lintrans::find_best_bsgs_ratio(diag, n, maxN, logMaxRatio);
    return HE_OK;
}
int he_lintrans_galois_elements(he_handle hev, const int *diag, int n, int slots, int logBSGSRatio, uint64_t *out, size_t cap, size_t *n_out) {
    static const char *who = "he_lintrans_galois_elements";
    GET(ev, Evaluator, hev, T_EVAL);
    if (n < 0 || (n > 0 && !diag) || !n_out || (cap && !out)) return fail(HE_EINVAL, "%s: null argument", who);
    if (slots < 1 || (slots & (slots - 1)) || logBSGSRatio > 30) return fail(HE_EINVAL, "%s: slots must be a power of two and logBSGSRatio at most 30", who);
    const BasisExtender &be = *ev->be;
    const std::vector<uint64_t> g = lintrans::galois_elements((uint64_t)2 << (be.Q->logN + be.type), diag, n, slots, logBSGSRatio);
    for (size_t i = 0; i < g.size() && i < cap; i++) out[i] = g[i];
    *n_out = g.size();
    return HE_OK;
}

namespace {
constexpr int kLintransGroups[3] = {1, 2, 4};
constexpr int kLintransDefaultGroup = 4;  // the fastest of 1, 2, 4 at the c5 shape (NOTES.md)
// one launch of the grouped kernel per ring part: where its rows start in the device table
struct LinTransGroupDev {
    size_t off = 0;
    int n_babies = 0, members = 0, terms_q = 0, terms_p = 0, babies_p = 0;
};
struct LinTrans : Obj {
    std::shared_ptr<Evaluator> ev;
    int levelQ = 0, levelP = 0, slots = 0, N1 = 0;
    std::atomic<int> group{0};                // he_lintrans_set_group (0: the default)
    std::vector<int> diag;                    // reduced
    std::vector<std::shared_ptr<Poly>> ptQ, ptP;
    lintrans::Plan plan[3];                   // for G = 1, 2, 4
    std::vector<LinTransGroupDev> gdev[3];
    uint64_t *d_tab = nullptr;                // the term tables of the three plans
    LinTrans() : Obj(T_LINTRANS) {}
    ~LinTrans() override {
        if (!d_tab) return;
        hipSetDevice(ev->be->ctx->dev);
        hipStreamSynchronize(ev->be->ctx->stream);
        hipFree(d_tab);
    }
};
int lintrans_default_group() {
    static const int g = [] {
        const char *s = getenv("HERING_LINTRANS_GROUP");
        const int v = s ? atoi(s) : 0;
        return (v == 1 || v == 2 || v == 4) ? v : kLintransDefaultGroup;
    }();
    return g;
}
inline int lintrans_group_slot(int G) { return G >= 4 ? 2 : (G >= 2 ? 1 : 0); }
// what one transformation of a call works with, resolved before the request is filed
struct LinTransJob {
    std::shared_ptr<LinTrans> lt;
    int levelQ = 0, gslot = 0;
    std::vector<std::shared_ptr<Evk>> giant_keys;  // BSGS: per giant step in plan order (null for j = 0); naive: per rotation
    std::vector<uint64_t> giant_gal;
    std::vector<size_t> slot_map;                  // BSGS: the call's pre-rotation slot of each non-zero baby step (empty: identity)
};
struct LinTransCall {
    std::shared_ptr<Evaluator> ev;
    int levelQd = 0, levelP = 0;
    std::vector<int> babies;                       // the call's non-zero baby steps, ascending: pre-rotation slot s holds babies[s]
    std::vector<std::shared_ptr<Evk>> baby_keys;
    std::vector<uint64_t> baby_gal;
    std::vector<LinTransJob> jobs;
    bool any_naive = false, any_bsgs = false;
    int max_group = 1;
};
inline uint64_t lintrans_overflow_half(const std::vector<uint64_t> &moduli, int level) {
    uint64_t mx = 0;
    for (int i = 0; i <= level; i++) mx = std::max(mx, moduli[(size_t)i]);
    return (uint64_t)(18446744073709551616.0 / (double)mx) >> 1;  // Qi/PiOverflowMargin(level) >> 1 (core/rlwe/params.go:554-570)
}
// scratch of the steps a call composes: the largest of what its entry points' launches reserve
size_t lintrans_step_words(const BasisExtender &be, int levelQ, int levelP, int B, const Evk *k) {
    return std::max({decompose_ntt_words(be, levelQ, B), auto_hoisted_lazy_words(be, levelQ, levelP, B),
                     giant_step_words(be, levelQ, levelP, B, k), eval_moddown_words(be, levelQ, levelP, B)}) + 64;
}
int lintrans_run(const LinTransCall &c, const View *v, int B) {
    const std::shared_ptr<Evaluator> &ev = c.ev;
    BasisExtender &be = *ev->be;
    Ctx &ctx = *be.ctx;
    hipStream_t st = ctx.stream;
    const int N = be.Q->N, levelQd = c.levelQd, levelP = c.levelP;
    const size_t b = (size_t)B, sQ = (size_t)(levelQd + 1) * N, sP = (size_t)(levelP + 1) * N;
    const int beta = base_rns_size(levelQd, levelP);
    const size_t dec_ds = (size_t)(be.LQ + be.LP) * N, dec_bs = (size_t)beta * dec_ds;
    const size_t nslots = c.babies.size();
    size_t map_words = 0;
    for (const LinTransJob &j : c.jobs) map_words += (j.slot_map.size() + 1) & ~(size_t)1;
    // the work block: the group's inner sums [G][2] QP (BSGS) or the key switch's accumulators [2] QP (naive)
    const size_t work = (size_t)std::max(c.any_bsgs ? c.max_group : 0, c.any_naive ? 1 : 0) * 2 * b * (sQ + sP);
    const size_t persistent = b * dec_bs + 2 * b * sQ + nslots * 2 * b * (sQ + sP) + (c.any_naive ? 2 * b * sQ : 0) + 2 * b * sP + work + map_words + 64;
    const Evk *k0 = !c.baby_keys.empty() ? c.baby_keys[0].get() : nullptr;
    for (const LinTransJob &j : c.jobs)
        for (const auto &k : j.giant_keys) if (!k0 && k) k0 = k.get();
    TRY(ctx.arena_reserve(persistent + lintrans_step_words(be, levelQd, levelP, B, k0)));
    const View decv{ctx.arena_take(b * dec_bs), dec_bs};
    uint64_t *pct = ctx.arena_take(2 * b * sQ);
    uint64_t *preQ = ctx.arena_take(nslots * 2 * b * sQ), *preP = ctx.arena_take(nslots * 2 * b * sP);
    uint64_t *cp = c.any_naive ? ctx.arena_take(2 * b * sQ) : nullptr;
    uint64_t *accP = ctx.arena_take(2 * b * sP);
    uint64_t *workQ = ctx.arena_take(work / (sQ + sP) * sQ), *workP = ctx.arena_take(work / (sQ + sP) * sP);
    const View c0P{accP, sP}, c1P{accP + b * sP, sP};
    const View pct0{pct, sQ}, pct1{pct + b * sQ, sQ};
    const LimbTab tqd = ident_tab(levelQd + 1);
    // ONE DecomposeNTT of c1 at levelQd with levelP + 1 special primes (:52)
    {
        Ctx::ArenaFrame f(ctx);
        const View vv[2] = {v[1], decv};
        TRY(decompose_ntt_run(ev, levelQd, levelP, levelP + 1, 1, dec_ds, vv, B));
    }
    // P * ct (BSGS :316-317; the naive form's P * c0 :190) and the naive form's copy of the input (:175-176)
    {
        ScalarTab s{};
        for (int i = 0; i <= levelQd; i++) {
            const ModConst &m = be.Q->sub[i].mc;
            uint64_t pm = 1;
            for (int j = 0; j <= levelP; j++) pm = mulmod(pm, be.P->moduli[j] % m.q, m.q);
            s.s[i] = mform(pm, m.q, m.brc0, m.brc1);
        }
        const double comps = c.any_bsgs ? 2.0 : 1.0;  // (the naive form multiplies c0 only)
        ctx.acct(2.0 * comps * (levelQd + 1), 0, B, N);
        { Valu V(be.Q->logN); for (int i = 0; i <= levelQd; i++) V.mul(cls_f64(be.small, i), comps); V.into(ctx, B); }
        HIP_TRY(launch_ew(be.qp, tqd, EW_MUL_SCALAR_MONT, v[0], v[0], pct0, B, &s, nullptr, st));
        if (c.any_bsgs) HIP_TRY(launch_ew(be.qp, tqd, EW_MUL_SCALAR_MONT, v[1], v[1], pct1, B, &s, nullptr, st));
        if (cp) {
            ctx.acct(4.0 * (levelQd + 1), 0, B, N);
            for (int k = 0; k < 2; k++)  // (plain views: the request is served alone)
                HIP_TRY(hipMemcpy2DAsync(cp + (size_t)k * b * sQ, sQ * 8, v[k].p, v[k].bstride * 8, sQ * 8, B, hipMemcpyDeviceToDevice, st));
        }
    }
    // the pre-rotations every BSGS transformation of the call shares (:62, :82-104): AutomorphismHoistedLazy at levelQd
    for (size_t s = 0; s < nslots; s++) {
        Ctx::ArenaFrame f(ctx);
        const View vv[6] = {v[0], decv, View{preQ + s * 2 * b * sQ, sQ}, View{preP + s * 2 * b * sP, sP},
                            View{preQ + (s * 2 + 1) * b * sQ, sQ}, View{preP + (s * 2 + 1) * b * sP, sP}};
        TRY(auto_hoisted_lazy_run(ev, c.baby_keys[s], levelQd, levelP, c.baby_gal[s], KsAlias{}, dec_ds, vv, B));
    }
    for (size_t t = 0; t < c.jobs.size(); t++) {
        const LinTransJob &job = c.jobs[t];
        const LinTrans &lt = *job.lt;
        const int lq = job.levelQ;
        const View out0 = v[2 + 2 * t], out1 = v[3 + 2 * t];
        const LimbTab tq = ident_tab(lq + 1), tp = ident_tab(levelP + 1, 0, 0, be.LQ);
        const lintrans::Plan &plan = lt.plan[job.gslot];
        auto moddown = [&](View q, View p) -> int {
            Ctx::ArenaFrame f(ctx);
            const View vv[3] = {q, p, q};
            return eval_moddown_run(ev, lq, levelP, vv, B);
        };
        if (lt.N1 == 0) {
            // MultiplyByDiagMatrix (:142-274).  The accumulators stay canonical (launch_diag_mac), so the reference's periodic
            // Reduce calls are no-ops here.
            const View cQ0{workQ, sQ}, cQ1{workQ + b * sQ, sQ}, cP0{workP, sP}, cP1{workP + b * sP, sP};
            const View cp0{cp, sQ}, cp1{cp + b * sQ, sQ};
            for (size_t r = 0; r < plan.rotations.size(); r++) {
                const Evk &k = *job.giant_keys[r];
                const uint32_t *index = nullptr;
                TRY(cached_auto_index(*ev, job.giant_gal[r], &index));
                ctx.acct(key_limbs(k, lq) / 2 + 2.0 * (lq + levelP + 2), key_limbs(k, lq), B, N);  // he_gadget_product_hoisted_lazy
                { Valu V(be.Q->logN); valu_keyswitch(V, be, lq, levelP, base_rns_size(lq, levelP), false, true); V.into(ctx, B); }
                TRY(ks_inner(*ev, lq, levelP, decv, dec_ds, k, cQ0, cP0, cQ1, cP1, B));
                ctx.acct(3.0 * (lq + 1), 0, B, N);
                HIP_TRY(launch_ew(be.qp, tq, EW_ADD, cQ0, pct0, cQ0, B, nullptr, nullptr, st));  // + P * c0 before the automorphism (:221)
                const Poly &dq = *lt.ptQ[(size_t)plan.rotation_term[r]], &dp = *lt.ptP[(size_t)plan.rotation_term[r]];
                DiagMacArgs aq{}, ap{};
                aq.n = ap.n = 1; aq.nlimbs = lq + 1; ap.nlimbs = levelP + 1; aq.accumulate = ap.accumulate = r > 0 ? 1 : 0;
                aq.mod0 = 0; ap.mod0 = be.LQ;
                aq.pt[0] = dq.d; aq.c0[0] = cQ0.p; aq.c1[0] = cQ1.p; aq.c0_bs[0] = aq.c1_bs[0] = sQ; aq.index[0] = index;
                ap.pt[0] = dp.d; ap.c0[0] = cP0.p; ap.c1[0] = cP1.p; ap.c0_bs[0] = ap.c1_bs[0] = sP; ap.index[0] = index;
                ctx.acct((r > 0 ? 6.0 : 4.0) * (lq + levelP + 2), (double)(lq + levelP + 2), B, N);
                { Valu V(be.Q->logN); for (int i = 0; i <= lq; i++) V.mul(cls_f64(be.small, i), 4.0); for (int j = 0; j <= levelP; j++) V.mul(cls_f64(be.small, be.LQ + j), 4.0); V.into(ctx, B); }
                HIP_TRY(launch_diag_mac(be.qp, aq, out0, out1, B, st));
                HIP_TRY(launch_diag_mac(be.qp, ap, c0P, c1P, B, st));
            }
            if (!plan.rotations.empty()) {
                TRY(moddown(out0, c0P));
                TRY(moddown(out1, c1P));
            }
            // the zero diagonal after the ModDown, on the Q part only (:266-272); a transformation with no other diagonal is that
            // product alone (no rotation has written the accumulators)
            const bool fresh = plan.rotations.empty();
            ctx.acct((fresh ? 4.0 : 6.0) * (lq + 1), (double)(lq + 1), B, N);
            if (plan.zero_diag >= 0) {
                { Valu V(be.Q->logN); for (int i = 0; i <= lq; i++) V.mul(cls_f64(be.small, i), 2.0); V.into(ctx, B); }
                const View pt{lt.ptQ[(size_t)plan.zero_diag]->d, 0};
                const int op = fresh ? EW_MUL_MONT : EW_MUL_MONT_THEN_ADD;
                HIP_TRY(launch_ew(be.qp, tq, op, pt, cp0, out0, B, nullptr, nullptr, st));
                HIP_TRY(launch_ew(be.qp, tq, op, pt, cp1, out1, B, nullptr, nullptr, st));
            } else if (fresh) {
                HIP_TRY(launch_ew(be.qp, tq, EW_ZERO, out0, out0, out0, B, nullptr, nullptr, st));
                HIP_TRY(launch_ew(be.qp, tq, EW_ZERO, out1, out1, out1, B, nullptr, nullptr, st));
            }
            continue;
        }
        // MultiplyByDiagMatrixBSGS (:280-469)
        const uint64_t *slot_map = nullptr;
        if (!job.slot_map.empty()) {
            size_t *m = reinterpret_cast<size_t *>(ctx.arena_take(job.slot_map.size()));
            HIP_TRY(launch_tab_fill(m, job.slot_map.data(), (int)job.slot_map.size(), st));
            slot_map = reinterpret_cast<const uint64_t *>(m);
        }
        const uint64_t QiOverF = lintrans_overflow_half(be.Q->moduli, lq), PiOverF = lintrans_overflow_half(be.P->moduli, levelP);
        uint64_t cnt0 = 0;
        size_t giant = 0;
        auto reduce = [&](bool onQ) -> int {
            ctx.acct(4.0 * (onQ ? lq + 1 : levelP + 1), 0, B, N);
            if (onQ) {
                HIP_TRY(launch_ew(be.qp, tq, EW_REDUCE, out0, out0, out0, B, nullptr, nullptr, st));
                HIP_TRY(launch_ew(be.qp, tq, EW_REDUCE, out1, out1, out1, B, nullptr, nullptr, st));
            } else {
                HIP_TRY(launch_ew(be.qp, tp, EW_REDUCE, c0P, c0P, c0P, B, nullptr, nullptr, st));
                HIP_TRY(launch_ew(be.qp, tp, EW_REDUCE, c1P, c1P, c1P, B, nullptr, nullptr, st));
            }
            return HE_OK;
        };
        for (size_t g = 0; g < plan.groups.size(); g++) {
            const lintrans::Group &grp = plan.groups[g];
            const LinTransGroupDev &gd = lt.gdev[job.gslot][g];
            // the inner sums of the group's members (:342-394), canonical: ONE launch per ring part
            DiagMacGroupArgs a{};
            a.tab = lt.d_tab + gd.off; a.n_babies = gd.n_babies; a.members = gd.members; a.row_words = 1 + 2 * gd.members;
            a.slot_map = slot_map;
            a.out_member = 2 * b; a.out_comp = b;  // (x the part's entry stride, below)
            DiagMacGroupArgs aq = a, ap = a;
            aq.part = 0; aq.ct = preQ; aq.ct_slot = 2 * b * sQ; aq.ct_comp = b * sQ; aq.ct_bs = sQ;
            aq.pct = pct; aq.pct_comp = b * sQ; aq.pct_bs = sQ;
            aq.out = workQ; aq.out_member *= sQ; aq.out_comp *= sQ; aq.out_bs = sQ; aq.nlimbs = lq + 1; aq.mod0 = 0; aq.terms = gd.terms_q;
            ap.part = 1; ap.ct = preP; ap.ct_slot = 2 * b * sP; ap.ct_comp = b * sP; ap.ct_bs = sP;
            ap.pct = nullptr;  // the i = 0 term is P * ct with no P part (:349-352)
            ap.out = workP; ap.out_member *= sP; ap.out_comp *= sP; ap.out_bs = sP; ap.nlimbs = levelP + 1; ap.mod0 = be.LQ; ap.terms = gd.terms_p;
            // giant step j = 0 comes first (the giant steps ascend) and opens the outer accumulators with a copy (:425-433): its
            // inner sums are written where that copy would put them
            const bool opens = cnt0 == 0 && grp.giants[0] == 0;
            if (opens) {
                aq.m0[0] = out0.p; aq.m0[1] = out1.p; aq.m0_bs[0] = out0.bstride; aq.m0_bs[1] = out1.bstride;
                ap.m0[0] = c0P.p; ap.m0[1] = c1P.p; ap.m0_bs[0] = ap.m0_bs[1] = sP;
            }
            ctx.acct((2.0 * gd.n_babies + 2.0 * gd.members) * (lq + 1) + (2.0 * gd.babies_p + 2.0 * gd.members) * (levelP + 1),
                     (double)gd.terms_q * (lq + 1) + (double)gd.terms_p * (levelP + 1), B, N);
            {
                Valu V(be.Q->logN);
                for (int i = 0; i <= lq; i++) V.mul(cls_f64(be.small, i), 2.0 * gd.terms_q + 2.0 * gd.members);
                for (int j = 0; j <= levelP; j++) V.mul(cls_f64(be.small, be.LQ + j), 2.0 * gd.terms_p + 2.0 * gd.members);
                V.into(ctx, B);
            }
            HIP_TRY(launch_diag_mac_group(be.qp, aq, B, st));
            HIP_TRY(launch_diag_mac_group(be.qp, ap, B, st));
            for (int m = 0; m < gd.members; m++, giant++) {
                const View t0Q{workQ + (size_t)(2 * m) * b * sQ, sQ}, t1Q{workQ + (size_t)(2 * m + 1) * b * sQ, sQ};
                const View t0P{workP + (size_t)(2 * m) * b * sP, sP}, t1P{workP + (size_t)(2 * m + 1) * b * sP, sP};
                if (grp.giants[(size_t)m] != 0) {
                    TRY(moddown(t1Q, t1P));  // the hoisted ModDown of sum(sum(phi(d1) * plaintext)) (:397)
                    Ctx::ArenaFrame f(ctx);
                    const View vv[7] = {t1Q, t0Q, t0P, out0, c0P, out1, c1P};
                    TRY(giant_step_run(ev, job.giant_keys[giant], lq, levelP, job.giant_gal[giant], cnt0 != 0, vv, B));
                } else if (!(opens && m == 0)) {
                    // (the giant steps ascend and are distinct: j = 0 can only be the first member of the first group)
                    return fail(HE_EINVAL, "internal error: giant step 0 is not the first of the plan");
                }
                if (cnt0 % QiOverF == QiOverF - 1) TRY(reduce(true));   // :443-453
                if (cnt0 % PiOverF == PiOverF - 1) TRY(reduce(false));
                cnt0++;
            }
        }
        if (cnt0 % QiOverF != 0) TRY(reduce(true));   // :456-464
        if (cnt0 % PiOverF != 0) TRY(reduce(false));
        TRY(moddown(out0, c0P));  // sum(phi(c0 * P + d0_QP)) / P
        TRY(moddown(out1, c1P));  // sum(phi(d1_QP)) / P
    }
    return HE_OK;
}
}  // namespace

int he_lintrans_create(he_handle hev, int levelQ, int levelP, int log_slots, int N1, int n, const int *diag, const he_handle *ptQ,
                       const he_handle *ptP, he_handle *out) {
    static const char *who = "he_lintrans_create";
    GET(ev, Evaluator, hev, T_EVAL);
    BasisExtender &be = *ev->be;
    if (!out || n < 1 || !diag || !ptQ || !ptP) return fail(HE_EINVAL, "%s: at least one diagonal, its polynomials and an output are needed", who);
    if (levelQ < 0 || levelQ >= be.LQ || levelP < 0 || levelP >= be.LP) return fail(HE_EINVAL, "%s: level out of range", who);
    if (log_slots < 0 || log_slots > be.Q->logN) return fail(HE_EINVAL, "%s: log_slots out of range", who);
    const int slots = 1 << log_slots;
    if (N1 < 0 || (N1 & (N1 - 1))) return fail(HE_EINVAL, "%s: N1 must be 0 (naive) or a power of two", who);
    auto lt = std::make_shared<LinTrans>();
    lt->ev = ev; lt->levelQ = levelQ; lt->levelP = levelP; lt->slots = slots; lt->N1 = N1;
    for (int k = 0; k < n; k++) {
        int d = diag[k] & (slots - 1);
        if (d < 0) d += slots;
        if (std::find(lt->diag.begin(), lt->diag.end(), d) != lt->diag.end())
            return fail(HE_EINVAL, "%s: diagonal %d (index %d) reduces to rotation %d, which is listed already", who, k, diag[k], d);
        std::shared_ptr<Poly> q = get<Poly>(ptQ[k], T_POLY), p = get<Poly>(ptP[k], T_POLY);
        if (!q || !p) return fail(HE_EHANDLE, "%s: bad Poly handle (diagonal %d)", who, k);
        if (q->ctx != be.ctx || p->ctx != be.ctx || q->N != be.Q->N || p->N != be.Q->N)
            return fail(HE_EINVAL, "%s: diagonal %d belongs to another context or degree", who, k);
        if (q->nlimbs < levelQ + 1 || p->nlimbs < levelP + 1) return fail(HE_EINVAL, "%s: diagonal %d has too few limbs", who, k);
        if (q->batch != 1 || p->batch != 1) return fail(HE_EINVAL, "%s: diagonal %d must be a polynomial of one entry", who, k);
        if (q->d == p->d) return fail(HE_EINVAL, "%s: diagonal %d names one polynomial for its Q and its P part", who, k);
        lt->diag.push_back(d); lt->ptQ.push_back(q); lt->ptP.push_back(p);
    }
    const uint64_t nth_root = (uint64_t)2 << (be.Q->logN + be.type);
    std::vector<uint64_t> tab;
    for (int s = 0; s < 3; s++) {
        if (!lintrans::build_plan(lt->diag.data(), n, slots, N1, kLintransGroups[s], nth_root, &lt->plan[s]))
            return fail(HE_EINVAL, "%s: no plan for these diagonals", who);
        const lintrans::Plan &p = lt->plan[s];
        std::vector<int> nz;  // the non-zero baby steps: pre-rotation number 1 + position
        for (int i : p.babies) if (i != 0) nz.push_back(i);
        for (const lintrans::Group &g : p.groups) {
            LinTransGroupDev gd;
            gd.off = tab.size(); gd.n_babies = (int)g.babies.size(); gd.members = (int)g.giants.size();
            for (size_t bs = 0; bs < g.babies.size(); bs++) {
                const int i = g.babies[bs];
                tab.push_back(i == 0 ? 0 : (uint64_t)(1 + (std::lower_bound(nz.begin(), nz.end(), i) - nz.begin())));
                if (i != 0) gd.babies_p++;
                for (int m = 0; m < gd.members; m++) {
                    const int t = g.term[bs * (size_t)gd.members + m];
                    tab.push_back(t < 0 ? 0 : (uint64_t)(uintptr_t)lt->ptQ[(size_t)t]->d);
                    tab.push_back(t < 0 ? 0 : (uint64_t)(uintptr_t)lt->ptP[(size_t)t]->d);
                    if (t >= 0) { gd.terms_q++; if (i != 0) gd.terms_p++; }
                }
            }
            lt->gdev[s].push_back(gd);
        }
    }
    if (!tab.empty()) {
        Scope sc(be.ctx.get());
        HIP_TRY(hipMalloc((void **)&lt->d_tab, tab.size() * sizeof(uint64_t)));
        HIP_TRY(hipMemcpy(lt->d_tab, tab.data(), tab.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    *out = reg(lt);
    return HE_OK;
}
int he_lintrans_destroy(he_handle h) { return unreg(h, T_LINTRANS); }
int he_lintrans_set_group(he_handle h, int G) {
    GET(lt, LinTrans, h, T_LINTRANS);
    if (G != 0 && G != 1 && G != 2 && G != 4) return fail(HE_EINVAL, "he_lintrans_set_group: G must be 0 (the default), 1, 2 or 4");
    lt->group.store(G);
    return HE_OK;
}

int he_lintrans_evaluate_many(he_handle hev, he_handle hset, int ct_level, he_handle hin0, he_handle hin1, int n_lt, const he_handle *lts,
                              const he_handle *out0, const he_handle *out1) {
    static const char *who = "he_lintrans_evaluate_many";
    GET(ev, Evaluator, hev, T_EVAL);
    std::shared_ptr<GaloisSet> set;  // (0: no key set -- transformations of the zero diagonal alone need none)
    if (hset) { set = get<GaloisSet>(hset, T_GALOIS_SET); if (!set) return fail(HE_EHANDLE, "%s: bad Galois key set handle", who); }
    BasisExtender &be = *ev->be;
    if (n_lt < 1 || !lts || !out0 || !out1) return fail(HE_EINVAL, "%s: at least one transformation and its outputs are needed", who);
    if (set && set->ev.get() != ev.get()) return fail(HE_EINVAL, "%s: the key set belongs to another evaluator", who);
    TRY(check_level(*be.Q, ct_level, who));
    auto call = std::make_shared<LinTransCall>();
    call->ev = ev;
    int maxQ = 0;
    for (int t = 0; t < n_lt; t++) {
        std::shared_ptr<LinTrans> lt = get<LinTrans>(lts[t], T_LINTRANS);
        if (!lt) return fail(HE_EHANDLE, "%s: bad LinearTransformation handle (transformation %d)", who, t);
        if (lt->ev.get() != ev.get()) return fail(HE_EINVAL, "%s: transformation %d belongs to another evaluator", who, t);
        if (t == 0) call->levelP = lt->levelP;
        else if (lt->levelP != call->levelP) return fail(HE_EINVAL, "%s: all linearTransformations must have the same levelP", who);
        maxQ = std::max(maxQ, lt->levelQ);
        LinTransJob job;
        job.lt = lt;
        call->jobs.push_back(std::move(job));
    }
    const int levelQd = call->levelQd = std::min(maxQ, ct_level), levelP = call->levelP;
    CoReq q;
    Operands o(q, who, be);
    const int i0 = o.in(hin0, ct_level + 1, "in0"), i1 = o.in(hin1, ct_level + 1, "in1");
    for (int t = 0; t < n_lt; t++) {
        LinTransJob &job = call->jobs[(size_t)t];
        const std::shared_ptr<Poly> p0 = o.poly(out0[t]);
        job.levelQ = std::min({p0 ? p0->nlimbs - 1 : 0, ct_level, job.lt->levelQ});
        const int a = o.out(p0, job.levelQ + 1, "out0"), c = o.out(out1[t], job.levelQ + 1, "out1");
        if (n_lt == 1) { o.inplace(a, i0); o.inplace(a, i1); o.inplace(c, i0); o.inplace(c, i1); }
    }
    for (const LinTransJob &job : call->jobs)
        for (size_t k = 0; k < job.lt->ptQ.size(); k++) {
            o.in(job.lt->ptQ[k], job.lt->levelQ + 1, "diagonal (Q)", Operands::kBroadcast);
            o.inP(job.lt->ptP[k], levelP + 1, "diagonal (P)", Operands::kBroadcast);
        }
    TRY(o.check());
    const int B = o.B;
    // the keys: every element the plans ask for, present, of the transformations' LevelP, reaching the level it is used at
    auto key_of = [&](uint64_t gal, int level, std::shared_ptr<Evk> *k) -> int {
        const int at = set ? set->find(reduce_gal(gal, be.Q->logN, be.type)) : -1;
        if (at < 0) return fail(HE_EINVAL, "%s: the key set has no key for Galois element %llu", who, (unsigned long long)gal);
        *k = set->keys[(size_t)at];
        if ((*k)->nPk - 1 != levelP)
            return fail(HE_EINVAL, "%s: LinearTransformation.LevelP = %d != GaloisKey[%llu].LevelP() = %d", who, levelP, (unsigned long long)gal, (*k)->nPk - 1);
        if ((*k)->pw2) return fail(HE_EINVAL, "%s: method is unsupported for BaseTwoDecomposition != 0", who);
        if ((*k)->nQk - 1 < level) return fail(HE_EINVAL, "%s: the key of Galois element %llu stops at level %d, %d needed", who, (unsigned long long)gal, (*k)->nQk - 1, level);
        return HE_OK;
    };
    const uint64_t nth_root = (uint64_t)2 << (be.Q->logN + be.type);
    std::set<int> babies;
    for (const LinTransJob &job : call->jobs)
        if (job.lt->N1 != 0) for (int i : job.lt->plan[0].babies) if (i != 0) babies.insert(i);
    call->babies.assign(babies.begin(), babies.end());
    for (int i : call->babies) {
        std::shared_ptr<Evk> k;
        const uint64_t gal = lintrans::galois_element(nth_root, i);
        TRY(key_of(gal, levelQd, &k));
        call->baby_keys.push_back(k); call->baby_gal.push_back(reduce_gal(gal, be.Q->logN, be.type));
    }
    // the scratch of the call without the group block (lintrans_run): a group may take as much again at most -- G is halved
    // while its [G][2] QP block is larger
    const size_t N = be.Q->N, sQP = (size_t)(levelQd + levelP + 2) * N;
    const size_t rest = (size_t)B * ((size_t)base_rns_size(levelQd, levelP) * (be.LQ + be.LP) * N + (2 + 2 * call->babies.size()) * sQP);
    for (LinTransJob &job : call->jobs) {
        const LinTrans &lt = *job.lt;
        if (lt.N1 == 0) {
            call->any_naive = true;
            const lintrans::Plan &p = lt.plan[0];
            for (size_t r = 0; r < p.rotations.size(); r++) {
                std::shared_ptr<Evk> k;
                TRY(key_of(p.galois[r], job.levelQ, &k));
                job.giant_keys.push_back(k); job.giant_gal.push_back(reduce_gal(p.galois[r], be.Q->logN, be.type));
            }
            continue;
        }
        call->any_bsgs = true;
        int G = lt.group.load();
        if (G == 0) G = lintrans_default_group();
        while (G > 1 && (size_t)G * 2 * B * sQP > rest) G >>= 1;
        job.gslot = lintrans_group_slot(G);
        call->max_group = std::max(call->max_group, G);
        for (const lintrans::Group &g : lt.plan[job.gslot].groups)
            for (int j : g.giants) {
                std::shared_ptr<Evk> k;
                const uint64_t gal = j != 0 ? lintrans::galois_element(nth_root, j) : 1;
                if (j != 0) TRY(key_of(gal, job.levelQ, &k));
                job.giant_keys.push_back(k); job.giant_gal.push_back(reduce_gal(gal, be.Q->logN, be.type));
            }
        std::vector<int> nz;
        for (int i : lt.plan[0].babies) if (i != 0) nz.push_back(i);
        if (nz != call->babies)
            for (int i : nz) job.slot_map.push_back((size_t)(std::lower_bound(call->babies.begin(), call->babies.end(), i) - call->babies.begin()));
    }
    q.op = CO_LINTRANS_EVAL; q.obj = ev.get(); q.key = set.get(); q.par[0] = ct_level; q.par[1] = n_lt;
    for (const LinTransJob &job : call->jobs) { q.blob.push_back((uint64_t)(uintptr_t)job.lt.get()); q.blob.push_back((uint64_t)job.gslot); q.keep.push_back(job.lt); }
    q.keep.push_back(ev);
    if (set) q.keep.push_back(set);
    q.run = [call](const View *v, int B) -> int { return lintrans_run(*call, v, B); };
    q.one_by_one();  // (scratch-to-scratch launches: no entry tables)
    return co_dispatch(*be.ctx, B, q);
}
int he_lintrans_evaluate(he_handle ev, he_handle set, int ct_level, he_handle in0, he_handle in1, he_handle lt, he_handle out0, he_handle out1) {
    return he_lintrans_evaluate_many(ev, set, ct_level, in0, in1, 1, &lt, &out0, &out1);
}
int he_debug_lintrans_plan(uint64_t nth_root, int slots, int N1, int G, int n, const int *diag, int64_t *out, size_t cap, size_t *n_words) {
    static const char *who = "he_debug_lintrans_plan";
    if (!n_words || n < 0 || (n > 0 && !diag) || (cap && !out)) return fail(HE_EINVAL, "%s: null argument", who);
    lintrans::Plan p;
    if (!lintrans::build_plan(diag, n, slots, N1, G, nth_root, &p))
        return fail(HE_EINVAL, "%s: slots, N1 and NthRoot must be powers of two, G in [1, %d], the diagonals reduced and distinct", who, lintrans::kMaxGroup);
    const std::vector<int64_t> w = lintrans::plan_words(p);
    for (size_t i = 0; i < w.size() && i < cap; i++) out[i] = w[i];
    *n_words = w.size();
    return HE_OK;
}

// ---------------------------------------------------------------------------------------
// polynomial.Evaluator (include/hering_polyeval.h; circuits/common/polynomial): the integer logic on the host
// (csrc/polyeval_plan.h), the Polynomial handle with the caller's scalar words, and the baby steps through the leaf-group kernel
// ---------------------------------------------------------------------------------------
int he_polyeval_optimal_split(int log_degree, int *log_split) {
    if (!log_split || log_degree < 1 || log_degree > 30) return fail(HE_EINVAL, "he_polyeval_optimal_split: log_degree must be in [1, 30]");
    *log_split = polyeval::optimal_split(log_degree);
    return HE_OK;
}
int he_polyeval_split_degree(int n, int *a, int *b) {
    if (!a || !b) return fail(HE_EINVAL, "he_polyeval_split_degree: null output");
    if (n <= 0) return fail(HE_EINVAL, "invalid n: n=%d should be greater than zero", n);
    polyeval::split_degree(n, a, b);
    return HE_OK;
}
int he_polyeval_depth(int degree, int level, int *depth) {
    if (degree < 1) return fail(HE_EINVAL, "he_polyeval_depth: the polynomial must have degree >= 1");
    const int d = polyeval::depth_of(degree);
    if (depth) *depth = d;
    if (level < d) return fail(HE_EINVAL, "%d levels < %d log(d) -> cannot evaluate poly", level, d);
    return HE_OK;
}

namespace {
constexpr int kPolyevalDefaultGroup = 4;
struct PolyevalPoly : Obj {
    std::shared_ptr<Ring> ring;
    polyeval::Plan plan;
    int L = 0;                     // limb stride of the scalar table: 1 + the level of X^1
    bool even = false, odd = false;
    std::map<int, polyeval::Power> planned_for;  // the basis the polynomial was planned for
    std::vector<uint32_t> off;     // per leaf: where its scalars start in the table
    std::atomic<int> group{0};     // he_polyeval_poly_set_group (0: the default)
    uint64_t *d_tab = nullptr;
    PolyevalPoly() : Obj(T_POLYEVAL) {}
    ~PolyevalPoly() override {
        if (!d_tab) return;
        hipSetDevice(ring->ctx->dev);
        hipStreamSynchronize(ring->ctx->stream);
        hipFree(d_tab);
    }
};
int polyeval_default_group() {
    static const int g = [] {
        const char *s = getenv("HERING_POLYEVAL_GROUP");
        const int v = s ? atoi(s) : 0;
        return (v == 1 || v == 2 || v == 4) ? v : kPolyevalDefaultGroup;
    }();
    return g;
}
int polyeval_present(const char *who, int n_powers, const int *powers, std::map<int, polyeval::Power> *out) {
    if (n_powers < 1 || !powers) return fail(HE_EINVAL, "%s: the powers the basis holds are needed (X^1 at least)", who);
    for (int i = 0; i < n_powers; i++) {
        const int n = powers[3 * i], level = powers[3 * i + 1], deg = powers[3 * i + 2];
        if (n < 1 || level < 0 || deg < 1 || deg > 2) return fail(HE_EINVAL, "%s: power %d: n >= 1, level >= 0 and degree 1 or 2 expected", who, i);
        if (!out->emplace(n, polyeval::Power{level, deg}).second) return fail(HE_EINVAL, "%s: X^{%d} is listed twice", who, n);
    }
    if (!out->count(1)) return fail(HE_EINVAL, "%s: cannot EvaluateFromPowerBasis: X^{1} is nil", who);
    return HE_OK;
}
// the caller's baby steps against the library's decomposition
int polyeval_check_leaves(const char *who, const polyeval::Plan &plan, int n_leaves, const int *leaf_degree, const int *leaf_level) {
    if (!plan.error.empty()) return fail(HE_EINVAL, "%s", plan.error.c_str());
    if (!leaf_degree || !leaf_level) return fail(HE_EINVAL, "%s: null argument", who);
    if (n_leaves != (int)plan.leaves.size()) return fail(HE_EINVAL, "%s: %d baby steps given, the decomposition has %d", who, n_leaves, (int)plan.leaves.size());
    for (int i = 0; i < n_leaves; i++) {
        const polyeval::Leaf &f = plan.leaves[(size_t)i];
        if (leaf_degree[i] != f.degree) return fail(HE_EINVAL, "%s: baby step %d has degree %d, the decomposition says %d", who, i, leaf_degree[i], f.degree);
        if (leaf_level[i] != f.level) return fail(HE_EINVAL, "%s: baby step %d is at level %d, the decomposition says %d", who, i, leaf_level[i], f.level);
    }
    return HE_OK;
}
}  // namespace

int he_polyeval_check_leaves(int degree, int basis, int even, int odd, int lazy, int n_powers, const int *powers, int n_leaves,
                             const int *leaf_degree, const int *leaf_level) {
    static const char *who = "he_polyeval_check_leaves";
    std::map<int, polyeval::Power> present;
    TRY(polyeval_present(who, n_powers, powers, &present));
    return polyeval_check_leaves(who, polyeval::build_plan(degree, basis, even != 0, odd != 0, lazy != 0, present, false), n_leaves, leaf_degree, leaf_level);
}
int he_polyeval_poly_create(he_handle hring, int degree, int basis, int even, int odd, int lazy, int n_powers, const int *powers,
                            int n_leaves, const int *leaf_degree, const int *leaf_level, const uint64_t *s0, const uint64_t *s1,
                            he_handle *out) {
    static const char *who = "he_polyeval_poly_create";
    GET(r, Ring, hring, T_RING);
    if (!out || !leaf_degree || !leaf_level || !s0 || !s1) return fail(HE_EINVAL, "%s: null argument", who);
    std::map<int, polyeval::Power> present;
    TRY(polyeval_present(who, n_powers, powers, &present));
    if (present[1].level >= r->nmod()) return fail(HE_EINVAL, "%s: X^1 at level %d on a ring of %d moduli", who, present[1].level, r->nmod());
    auto p = std::make_shared<PolyevalPoly>();
    p->ring = r; p->even = even != 0; p->odd = odd != 0; p->planned_for = present;
    p->plan = polyeval::build_plan(degree, basis, even != 0, odd != 0, lazy != 0, present, false);
    const std::vector<polyeval::Leaf> &leaves = p->plan.leaves;
    TRY(polyeval_check_leaves(who, p->plan, n_leaves, leaf_degree, leaf_level));
    const int L = p->L = present[1].level + 1;
    std::vector<uint64_t> tab;
    size_t at = 0;  // scalars consumed from s0 / s1
    for (int i = 0; i < n_leaves; i++) {
        const polyeval::Leaf &f = leaves[(size_t)i];
        if (f.level < 0 || f.level >= L) return fail(HE_EINVAL, "%s: baby step %d at level %d, outside [0, %d]", who, i, f.level, L - 1);
        if (f.degree > kPolyLeafMaxTerms) return fail(HE_EINVAL, "%s: baby step %d has %d terms, at most %d are admitted", who, i, f.degree, kPolyLeafMaxTerms);
        p->off.push_back((uint32_t)tab.size());
        for (int k = 0; k <= f.degree; k++, at++) {
            const bool has = (f.present >> k) & 1u;
            for (int h = 0; h < 2; h++) {
                const uint64_t *s = (h ? s1 : s0) + at * (size_t)L;
                for (int l = 0; l < L; l++) {
                    uint64_t w = 0;
                    if (has && l <= f.level) {
                        const ModConst &m = r->sub[(size_t)l].mc;
                        if (s[l] >= m.q) return fail(HE_EINVAL, "%s: baby step %d, term %d: the word of limb %d is not below the modulus", who, i, k, l);
                        w = k == 0 ? s[l] : mform(s[l], m.q, m.brc0, m.brc1);
                    }
                    tab.push_back(w);
                }
            }
        }
    }
    if (tab.size() >= ((size_t)1 << 32)) return fail(HE_EINVAL, "%s: the scalar table is too large", who);
    if (!tab.empty()) {
        Scope sc(r->ctx.get());
        HIP_TRY(hipMalloc((void **)&p->d_tab, tab.size() * sizeof(uint64_t)));
        HIP_TRY(hipMemcpy(p->d_tab, tab.data(), tab.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    }
    *out = reg(p);
    return HE_OK;
}
int he_polyeval_poly_destroy(he_handle h) { return unreg(h, T_POLYEVAL); }
int he_polyeval_poly_set_group(he_handle h, int G) {
    GET(p, PolyevalPoly, h, T_POLYEVAL);
    if (G != 0 && G != 1 && G != 2 && G != 4) return fail(HE_EINVAL, "he_polyeval_poly_set_group: G must be 0 (the default), 1, 2 or 4");
    p->group.store(G);
    return HE_OK;
}

int he_polyeval_leaves(he_handle hpoly, int first, int count, int n_powers, const he_handle *x, const he_handle *out) {
    static const char *who = "he_polyeval_leaves";
    GET(p, PolyevalPoly, hpoly, T_POLYEVAL);
    Ring &r = *p->ring;
    const std::vector<polyeval::Leaf> &leaves = p->plan.leaves;
    if (first < 0 || count < 1 || first + count > (int)leaves.size()) return fail(HE_EINVAL, "%s: baby steps [%d, %d) of %d", who, first, first + count, (int)leaves.size());
    if (n_powers < 0 || n_powers > kPolyLeafMaxTerms || (n_powers > 0 && !x) || !out) return fail(HE_EINVAL, "%s: at most %d powers, and the outputs, are needed", who, kPolyLeafMaxTerms);
    // the degree of each power given: its components must be 0 .. degree without a gap
    std::vector<int> xdeg((size_t)n_powers, -1);
    for (int k = 0; k < n_powers; k++) {
        for (int c = 0; c < 3; c++)
            if (x[3 * k + c]) {
                if (xdeg[(size_t)k] != c - 1) return fail(HE_EINVAL, "%s: X^{%d} has component %d without component %d", who, k + 1, c, c - 1);
                xdeg[(size_t)k] = c;
            }
        if (xdeg[(size_t)k] == 0) return fail(HE_EINVAL, "%s: X^{%d} is a plaintext: a ciphertext of degree 1 or 2 is expected", who, k + 1);
        const auto planned = p->plan.powers.find(k + 1);
        if (xdeg[(size_t)k] > 0 && planned != p->plan.powers.end() && planned->second.degree != xdeg[(size_t)k])
            return fail(HE_EINVAL, "%s: X^{%d} has degree %d, the polynomial was planned for degree %d", who, k + 1, xdeg[(size_t)k], planned->second.degree);
    }
    // What the reference's sequence leaves (MulThenAdd resizes its accumulator to the degree of each operand in turn,
    // schemes/ckks/evaluator.go:936 and schemes/bgv/evaluator.go:1118): the result has the degree of the LAST power used (the
    // lowest), and component c of power k survives only if every lower power used has that component too.  The leaves of one
    // polynomial use the powers its parity keeps, from the lowest up: which components of X^k survive is the same for all.
    std::vector<int> keepc((size_t)n_powers, -1);
    int need = 0, low = 2, lowest = 0;
    for (int g = 0; g < count; g++) need = std::max(need, leaves[(size_t)(first + g)].degree);
    for (int k = 1; k <= need; k++) {
        if (!polyeval::wanted(k, p->even, p->odd)) continue;
        if (k > n_powers || xdeg[(size_t)k - 1] < 0) return fail(HE_EINVAL, "%s: the baby steps need X^{%d}, which is not given", who, k);
        if (!lowest) lowest = k;
        low = std::min(low, xdeg[(size_t)k - 1]);
        keepc[(size_t)k - 1] = low;
    }
    std::vector<int> ctdeg((size_t)count);
    for (int g = 0; g < count; g++) {
        const polyeval::Leaf &f = leaves[(size_t)(first + g)];
        ctdeg[(size_t)g] = (f.present >> 1) ? xdeg[(size_t)lowest - 1] : f.ct_degree;
    }
    CoReq q;
    Operands o(q, who, r.ctx, r.N);
    // operands: [3 g + c] the outputs, then [3 count + 3 (k - 1) + c] the powers
    for (int g = 0; g < count; g++) {
        const polyeval::Leaf &f = leaves[(size_t)(first + g)];
        for (int c = 0; c < 3; c++) {
            const he_handle h = out[3 * g + c];
            if ((h != 0) != (c <= ctdeg[(size_t)g]))
                return fail(HE_EINVAL, "%s: the result of baby step %d has degree %d: component %d is %s", who, first + g, ctdeg[(size_t)g], c, h ? "not part of it" : "missing");
            o.out(o.opt(h), f.level + 1, "out");
        }
    }
    std::vector<int> xlevel((size_t)n_powers, -1);
    for (int g = 0; g < count; g++) {
        const polyeval::Leaf &f = leaves[(size_t)(first + g)];
        for (int k = 1; k <= f.degree && k <= n_powers; k++)
            if ((f.present >> k) & 1u) xlevel[(size_t)k - 1] = std::max(xlevel[(size_t)k - 1], f.level);
    }
    for (int k = 0; k < n_powers; k++)
        for (int c = 0; c < 3; c++) o.in(o.opt(x[3 * k + c]), xlevel[(size_t)k] + 1, "a power");
    TRY(o.check());
    const int B = o.B;
    int G = p->group.load();
    if (G == 0) G = polyeval_default_group();
    q.op = CO_POLY_LEAVES; q.obj = p.get(); q.par[0] = first; q.par[1] = count; q.par[2] = n_powers; q.par[3] = G;
    for (int k = 0; k < n_powers; k++) q.blob.push_back((uint64_t)(xdeg[(size_t)k] + 1));
    q.keep.push_back(p);
    q.run = [p, first, count, G, keepc](const View *v, int B) -> int {
        Ring &r = *p->ring;
        const std::vector<polyeval::Leaf> &leaves = p->plan.leaves;
        for (int g0 = 0; g0 < count; g0 += G) {
            PolyLeafGroupArgs a{};
            a.tab = p->d_tab; a.L = p->L; a.members = std::min(G, count - g0); a.ncomp = 2;
            int top = -1;
            for (int k = 0; k < kPolyLeafMaxTerms; k++) a.xlevel[k] = -1;
            // a power takes part as far as the members of THIS group use it
            for (int m = 0; m < a.members; m++) {
                const polyeval::Leaf &f = leaves[(size_t)(first + g0 + m)];
                a.off[m] = p->off[(size_t)(first + g0 + m)]; a.present[m] = f.present; a.level[m] = f.level;
                top = std::max(top, f.level);
                for (int c = 0; c < 3; c++) {
                    const View &ov = v[3 * (g0 + m) + c];
                    a.out[m][c] = ov.p; a.out_bs[m][c] = ov.bstride;
                    if (ov.p && c == 2) a.ncomp = 3;
                }
                for (int k = 1; k <= f.degree; k++)
                    if ((f.present >> k) & 1u) { a.n_powers = std::max(a.n_powers, k); a.xlevel[k - 1] = std::max(a.xlevel[k - 1], f.level); }
            }
            for (int k = 1; k <= a.n_powers; k++)
                for (int c = 0; c < 3; c++) {
                    const View &xv = v[3 * count + 3 * (k - 1) + c];
                    a.x[k - 1][c] = c <= keepc[(size_t)k - 1] ? xv.p : nullptr; a.x_bs[k - 1][c] = xv.bstride;
                }
            a.nlimbs = top + 1;
            double limbs = 0.0;
            for (int l = 0; l <= top; l++) {
                for (int k = 0; k < a.n_powers; k++) if (l <= a.xlevel[k]) for (int c = 0; c < 3; c++) limbs += a.x[k][c] ? 1.0 : 0.0;
                for (int m = 0; m < a.members; m++) if (l <= a.level[m]) for (int c = 0; c < 3; c++) limbs += a.out[m][c] ? 1.0 : 0.0;
            }
            r.ctx->acct(limbs, 0, B, r.N);
            HIP_TRY(launch_poly_leaf_group(r.dev, a, B, r.ctx->stream));
        }
        return HE_OK;
    };
    q.one_by_one();  // (the kernel takes no entry tables)
    return co_dispatch(*r.ctx, B, q);
}
// ---- PowerBasis and the whole evaluation: the library's plan run step by step, every step but the baby steps one of the operator
// entries of hering.h (each files its own request, in this thread's order, and records under a capture), the baby steps ONE
// he_polyeval_leaves call.  Everything that can be refused is refused before the first step is filed.
namespace {
struct PolyevalCt {
    std::vector<he_handle> v;  // degree + 1 polynomials, owned
    int level = 0;
};
struct PolyevalBasis : Obj {
    std::shared_ptr<Evaluator> ev;
    he_handle ev_h = 0, ring_h = 0;  // handles of its own on the evaluator and on its ring Q
    int basis = 0, batch = 1;
    std::mutex mu;
    std::map<int, PolyevalCt> X;
    PolyevalBasis() : Obj(T_POLYBASIS) {}
    ~PolyevalBasis() override {
        for (auto &kv : X) for (he_handle h : kv.second.v) he_poly_free(h);
        if (ev_h) unreg(ev_h, T_EVAL);
        if (ring_h) unreg(ring_h, T_RING);
    }
    std::map<int, polyeval::Power> held() const {
        std::map<int, polyeval::Power> m;
        for (const auto &kv : X) m[kv.first] = polyeval::Power{kv.second.level, (int)kv.second.v.size() - 1};
        return m;
    }
};
struct PolyevalAux {  // the caller's numbers for the Chebyshev steps, in the plan's order
    int n = 0;
    const int *kind = nullptr;  // 0: Add(x, -1); 1 / 2: Sub with the second / the first operand times the ratio first; 3: Sub as it is
    const uint64_t *s0 = nullptr, *s1 = nullptr;
    int L = 0;  // words per scalar
};
void polyeval_free(std::vector<he_handle> &v) {
    for (he_handle h : v) he_poly_free(h);
    v.clear();
}
int polyeval_alloc(PolyevalBasis &pb, int level, int n, std::vector<he_handle> *out) {
    for (int i = 0; i < n; i++) {
        he_handle h = 0;
        TRY(he_poly_alloc_scratch(pb.ring_h, level + 1, pb.batch, &h));
        out->push_back(h);
    }
    return HE_OK;
}
// what can be refused, before anything is filed
int polyeval_precheck(const char *who, PolyevalBasis &pb, const polyeval::Plan &plan, size_t first, bool bgv, he_handle rlk, const PolyevalAux &aux) {
    if (!plan.error.empty()) return fail(HE_EINVAL, "%s", plan.error.c_str());
    int n_aux = 0;
    const int top = pb.ev->be->Q->nmod() - 1;
    for (size_t i = first; i < plan.steps.size(); i++) {
        const polyeval::Step &s = plan.steps[i];
        if (s.level < 0 || s.level > top) return fail(HE_EINVAL, "%s: a step at level %d on a ring of %d moduli", who, s.level, top + 1);
        if ((s.op == polyeval::kRelinearize || s.op == polyeval::kMulRelinNew) && !rlk)
            return fail(HE_EINVAL, "%s: cannot relinearize: RelinearizationKey is nil", who);
        if (s.op == polyeval::kMul && s.degree == 1 && bgv) return fail(HE_EINVAL, "%s: cannot tensor: operands must be of degree 1", who);
        if (s.op == polyeval::kAddMinusOne || s.op == polyeval::kSub) {
            if (n_aux < aux.n) {
                const int k = aux.kind[n_aux];
                if ((s.op == polyeval::kAddMinusOne) != (k == 0) || k < 0 || k > 3)
                    return fail(HE_EINVAL, "%s: Chebyshev step %d of the plan is %s, the caller's kind is %d", who, n_aux, s.op == polyeval::kSub ? "a Sub" : "Add(x, -1)", k);
                if (k != 3 && (!aux.s0 || !aux.s1 || aux.L < s.level + 1)) return fail(HE_EINVAL, "%s: the words of Chebyshev step %d are missing", who, n_aux);
            }
            n_aux++;
        }
    }
    if (n_aux != aux.n) return fail(HE_EINVAL, "%s: the plan has %d Chebyshev constants and subtractions, the caller planned %d", who, n_aux, aux.n);
    if (rlk && !get<Evk>(rlk, T_EVK)) return fail(HE_EHANDLE, "%s: bad relinearization key handle", who);
    return HE_OK;
}
// steps [first, end) of the plan on the basis; poly_h: the planned polynomial (0: power steps only); out: the result's two outputs
int polyeval_exec(PolyevalBasis &pb, const polyeval::Plan &plan, size_t first, bool bgv, uint64_t t, he_handle rlk, const PolyevalAux &aux,
                  he_handle poly_h, const std::shared_ptr<PolyevalPoly> &poly, he_handle out0, he_handle out1) {
    std::map<int, PolyevalCt> leaves;
    int at_aux = 0;
    struct Cleanup {
        std::map<int, PolyevalCt> &l;
        ~Cleanup() { for (auto &kv : l) polyeval_free(kv.second.v); }
    } cleanup{leaves};
    auto ct = [&](int name) -> PolyevalCt & { return name > 0 ? pb.X[name] : leaves[name]; };
    auto tensor = [&](int level, const PolyevalCt &a, const PolyevalCt &b, bool relin, std::vector<he_handle> &o) -> int {
        if (a.v.size() != 2 || b.v.size() != 2) return fail(HE_EINVAL, "he_polyeval: cannot tensor: operands must be of degree 1");
        return bgv ? he_bgv_mul_relin(pb.ev_h, level, t, a.v[0], a.v[1], b.v[0], b.v[1], relin ? rlk : 0, o[0], o[1], relin ? 0 : o[2])
                   : he_ckks_mul_relin(pb.ev_h, level, a.v[0], a.v[1], b.v[0], b.v[1], relin ? rlk : 0, o[0], o[1], relin ? 0 : o[2]);
    };
    for (size_t i = first; i < plan.steps.size(); i++) {
        const polyeval::Step &s = plan.steps[i];
        const int lvl = s.level;
        switch (s.op) {
            case polyeval::kCopyNew: break;
            case polyeval::kNewCiphertext: {
                if (!leaves.empty()) break;
                const int n = (int)plan.leaves.size();
                int topdeg = 0;
                std::vector<he_handle> os((size_t)3 * n, 0);
                for (int g = 0; g < n; g++) {
                    const polyeval::Leaf &f = plan.leaves[(size_t)g];
                    PolyevalCt &c = leaves[-1 - g];
                    c.level = f.level;
                    TRY(polyeval_alloc(pb, f.level, f.ct_degree + 1, &c.v));
                    for (size_t k = 0; k < c.v.size(); k++) os[(size_t)3 * g + k] = c.v[k];
                    topdeg = std::max(topdeg, f.degree);
                }
                std::vector<he_handle> xs((size_t)3 * topdeg + 1, 0);
                for (int k = 1; k <= topdeg; k++) {
                    const auto it = pb.X.find(k);
                    if (it == pb.X.end()) continue;
                    for (size_t c = 0; c < it->second.v.size() && c < 3; c++) xs[(size_t)3 * (k - 1) + c] = it->second.v[c];
                }
                TRY(he_polyeval_leaves(poly_h, 0, n, topdeg, xs.data(), os.data()));
                break;
            }
            case polyeval::kAddConst: case polyeval::kMulThenAdd: break;
            case polyeval::kMulNew: case polyeval::kMulRelinNew: {
                const bool relin = s.op == polyeval::kMulRelinNew;
                std::vector<he_handle> o;
                TRY(polyeval_alloc(pb, lvl, relin ? 2 : 3, &o));
                const int rc = tensor(lvl, pb.X[s.a], pb.X[s.b], relin, o);
                if (rc != HE_OK) { polyeval_free(o); return rc; }
                PolyevalCt &x = pb.X[s.dst];
                x.v = o; x.level = lvl;
                break;
            }
            case polyeval::kRelinearize: {
                PolyevalCt &x = ct(s.dst);
                std::vector<he_handle> o;
                TRY(polyeval_alloc(pb, lvl, 2, &o));
                const int rc = x.v.size() == 3 ? he_relinearize(pb.ev_h, lvl, x.v[0], x.v[1], x.v[2], rlk, o[0], o[1]) : fail(HE_EINVAL, "he_polyeval: Relinearize of a ciphertext that is not of degree 2");
                if (rc != HE_OK) { polyeval_free(o); return rc; }
                polyeval_free(x.v);
                x.v = o; x.level = lvl;
                break;
            }
            case polyeval::kRescale: {
                PolyevalCt &x = ct(s.dst);
                const bool last = i + 1 == plan.steps.size() && out0 != 0;
                for (size_t c = 0; c < x.v.size(); c++) {
                    const he_handle dst = last ? (c == 0 ? out0 : out1) : x.v[c];
                    TRY(bgv ? he_div_round_by_last_modulus_ntt(pb.ring_h, lvl + 1, x.v[c], dst) : he_div_round_by_last_modulus_many_ntt(pb.ring_h, lvl + 1, 1, x.v[c], dst));
                }
                x.level = lvl;
                break;
            }
            case polyeval::kAddSelf: {
                PolyevalCt &x = ct(s.dst);
                for (he_handle h : x.v) TRY(he_add(pb.ring_h, lvl, h, h, h));
                x.level = lvl;
                break;
            }
            case polyeval::kAddMinusOne: {
                PolyevalCt &x = ct(s.dst);
                const size_t o = (size_t)at_aux++ * aux.L;
                TRY(he_double_rns_scalarop(pb.ring_h, lvl, 0, x.v[0], aux.s0 + o, aux.s1 + o, x.v[0]));
                x.level = lvl;
                break;
            }
            case polyeval::kSub: case polyeval::kAdd: {
                PolyevalCt &x = ct(s.dst);
                const PolyevalCt &y = ct(s.a);
                std::vector<he_handle> yv = y.v, scaled;
                if (s.op == polyeval::kSub) {
                    const int k = aux.kind[at_aux];
                    const size_t o = (size_t)at_aux++ * aux.L;
                    if (k == 1) {  // evaluateInPlace: the operand of the smaller scale times the integer ratio, into a new ciphertext
                        TRY(polyeval_alloc(pb, lvl, (int)y.v.size(), &scaled));
                        for (size_t c = 0; c < y.v.size(); c++) {
                            const int rc = he_double_rns_scalarop(pb.ring_h, lvl, 2, y.v[c], aux.s0 + o, aux.s1 + o, scaled[c]);
                            if (rc != HE_OK) { polyeval_free(scaled); return rc; }
                        }
                        yv = scaled;
                    } else if (k == 2) {
                        for (he_handle h : x.v) TRY(he_double_rns_scalarop(pb.ring_h, lvl, 2, h, aux.s0 + o, aux.s1 + o, h));
                    }
                }
                int rc = HE_OK;
                const size_t lo = std::min(x.v.size(), yv.size());
                for (size_t c = 0; c < lo && rc == HE_OK; c++)
                    rc = s.op == polyeval::kSub ? he_sub(pb.ring_h, lvl, x.v[c], yv[c], x.v[c]) : he_add(pb.ring_h, lvl, x.v[c], yv[c], x.v[c]);
                for (size_t c = lo; c < yv.size() && rc == HE_OK; c++) {  // the wider operand's further components: copied, negated for Sub
                    std::vector<he_handle> o;
                    rc = polyeval_alloc(pb, lvl, 1, &o);
                    if (rc == HE_OK) rc = s.op == polyeval::kSub ? he_neg(pb.ring_h, lvl, yv[c], o[0]) : he_poly_copy(o[0], yv[c], lvl);
                    if (rc == HE_OK) x.v.push_back(o[0]); else polyeval_free(o);
                }
                polyeval_free(scaled);
                TRY(rc);
                x.level = lvl;
                break;
            }
            case polyeval::kMul: {
                PolyevalCt &x = ct(s.dst);
                const PolyevalCt &y = pb.X[s.a];
                std::vector<he_handle> o;
                int rc;
                if (x.v.size() == 1) {  // a baby step of degree 0: plaintext x ciphertext (schemes/ckks/evaluator.go:842-870)
                    std::vector<he_handle> m;
                    TRY(polyeval_alloc(pb, lvl, 1, &m));
                    rc = polyeval_alloc(pb, lvl, (int)y.v.size(), &o);
                    if (rc == HE_OK) rc = he_mform(pb.ring_h, lvl, x.v[0], m[0]);
                    for (size_t c = 0; c < y.v.size() && rc == HE_OK; c++) rc = he_mul_coeffs_montgomery(pb.ring_h, lvl, m[0], y.v[c], o[c]);
                    polyeval_free(m);
                } else {
                    rc = polyeval_alloc(pb, lvl, 3, &o);
                    if (rc == HE_OK) rc = tensor(lvl, x, y, false, o);
                }
                if (rc != HE_OK) { polyeval_free(o); return rc; }
                polyeval_free(x.v);
                x.v = o; x.level = lvl;
                break;
            }
            default: return fail(HE_EINVAL, "he_polyeval: unknown step %d", s.op);
        }
    }
    (void)poly;
    return HE_OK;
}
int polyeval_aux(const char *who, int n_aux, const int *kind, const uint64_t *s0, const uint64_t *s1, int L, PolyevalAux *a) {
    if (n_aux < 0 || (n_aux > 0 && !kind)) return fail(HE_EINVAL, "%s: the kinds of the Chebyshev steps are missing", who);
    a->n = n_aux; a->kind = kind; a->s0 = s0; a->s1 = s1; a->L = L;
    return HE_OK;
}
}  // namespace

int he_polyeval_basis_create(he_handle hev, int basis, int level, he_handle in0, he_handle in1, he_handle *out) {
    static const char *who = "he_polyeval_basis_create";
    GET(ev, Evaluator, hev, T_EVAL);
    if (!out) return fail(HE_EINVAL, "%s: null output", who);
    if (basis != polyeval::kMonomial && basis != polyeval::kChebyshev) return fail(HE_EINVAL, "%s: unknown basis %d", who, basis);
    TRY(check_level(*ev->be->Q, level, who));
    std::shared_ptr<Poly> a = get<Poly>(in0, T_POLY), b = get<Poly>(in1, T_POLY);
    if (!a || !b) return fail(HE_EHANDLE, "%s: bad Poly handle", who);
    if (a->ctx != ev->be->ctx || b->ctx != ev->be->ctx || a->N != ev->be->Q->N || b->N != a->N) return fail(HE_EINVAL, "%s: the ciphertext belongs to another context or degree", who);
    if (a->nlimbs < level + 1 || b->nlimbs < level + 1 || a->batch != b->batch) return fail(HE_EINVAL, "%s: the ciphertext has too few limbs for level %d, or two batches", who, level);
    auto pb = std::make_shared<PolyevalBasis>();
    pb->ev = ev; pb->basis = basis; pb->batch = a->batch;
    pb->ev_h = reg(ev); pb->ring_h = reg(ev->be->Q);
    PolyevalCt x;
    x.level = level;
    TRY(polyeval_alloc(*pb, level, 2, &x.v));
    pb->X[1] = x;  // (owned from here on: a failure below releases it with the basis)
    TRY(he_poly_copy(x.v[0], in0, level));
    TRY(he_poly_copy(x.v[1], in1, level));
    *out = reg(pb);
    return HE_OK;
}
int he_polyeval_basis_destroy(he_handle h) { return unreg(h, T_POLYBASIS); }
int he_polyeval_basis_powers(he_handle h, int *powers, size_t cap, size_t *n) {
    GET(pb, PolyevalBasis, h, T_POLYBASIS);
    if (!n || (cap && !powers)) return fail(HE_EINVAL, "he_polyeval_basis_powers: null argument");
    std::lock_guard<std::mutex> lk(pb->mu);
    size_t i = 0;
    for (const auto &kv : pb->X) {
        if (i < cap) { powers[3 * i] = kv.first; powers[3 * i + 1] = kv.second.level; powers[3 * i + 2] = (int)kv.second.v.size() - 1; }
        i++;
    }
    *n = i;
    return HE_OK;
}
int he_polyeval_basis_power(he_handle h, int n, he_handle *comps) {
    GET(pb, PolyevalBasis, h, T_POLYBASIS);
    if (!comps) return fail(HE_EINVAL, "he_polyeval_basis_power: null output");
    std::lock_guard<std::mutex> lk(pb->mu);
    const auto it = pb->X.find(n);
    if (it == pb->X.end()) return fail(HE_EINVAL, "he_polyeval_basis_power: the basis holds no X^{%d}", n);
    for (size_t c = 0; c < 3; c++) comps[c] = c < it->second.v.size() ? it->second.v[c] : 0;
    return HE_OK;
}
int he_polyeval_gen_power(he_handle h, int scheme, uint64_t t, he_handle rlk, int n, int lazy, int n_aux, const int *aux_kind, const uint64_t *aux_s0,
                          const uint64_t *aux_s1, int aux_words) {
    static const char *who = "he_polyeval_gen_power";
    GET(pb, PolyevalBasis, h, T_POLYBASIS);
    if (n < 1) return fail(HE_EINVAL, "invalid n: n=%d should be greater than zero", n);
    if (scheme != 0 && scheme != 1) return fail(HE_EINVAL, "%s: scheme must be 0 (CKKS) or 1 (BGV)", who);
    std::lock_guard<std::mutex> lk(pb->mu);
    polyeval::Plan plan;
    plan.powers = pb->held();
    polyeval::gen_power(plan, pb->basis, n, lazy != 0);
    for (const polyeval::Step &s : plan.steps)
        if (s.level < 0) return fail(HE_EINVAL, "%s: X^{%d} would sink below level 0", who, n);
    PolyevalAux aux;
    TRY(polyeval_aux(who, n_aux, aux_kind, aux_s0, aux_s1, aux_words, &aux));
    TRY(polyeval_precheck(who, *pb, plan, 0, scheme == 1, rlk, aux));
    return polyeval_exec(*pb, plan, 0, scheme == 1, t, rlk, aux, 0, nullptr, 0, 0);
}
int he_polyeval_evaluate_from_power_basis(he_handle h, he_handle hpoly, int scheme, uint64_t t, he_handle rlk, int n_aux, const int *aux_kind,
                                          const uint64_t *aux_s0, const uint64_t *aux_s1, int aux_words, he_handle out0, he_handle out1) {
    static const char *who = "he_polyeval_evaluate_from_power_basis";
    GET(pb, PolyevalBasis, h, T_POLYBASIS);
    GET(p, PolyevalPoly, hpoly, T_POLYEVAL);
    if (scheme != 0 && scheme != 1) return fail(HE_EINVAL, "%s: scheme must be 0 (CKKS) or 1 (BGV)", who);
    if (p->ring.get() != pb->ev->be->Q.get()) return fail(HE_EINVAL, "%s: the polynomial was planned on another ring", who);
    std::lock_guard<std::mutex> lk(pb->mu);
    // the basis must be the one the polynomial was planned for: the same powers at the same levels and degrees
    const std::map<int, polyeval::Power> held = pb->held();
    if (held.size() != p->planned_for.size()) return fail(HE_EINVAL, "%s: the basis holds %zu powers, the polynomial was planned for %zu", who, held.size(), p->planned_for.size());
    for (const auto &kv : held) {
        const auto it = p->planned_for.find(kv.first);
        if (it == p->planned_for.end() || it->second.level != kv.second.level || it->second.degree != kv.second.degree)
            return fail(HE_EINVAL, "%s: X^{%d} of the basis (level %d, degree %d) is not what the polynomial was planned for", who, kv.first, kv.second.level, kv.second.degree);
    }
    const polyeval::Plan &plan = p->plan;
    PolyevalAux aux;
    TRY(polyeval_aux(who, n_aux, aux_kind, aux_s0, aux_s1, aux_words, &aux));
    TRY(polyeval_precheck(who, *pb, plan, 0, scheme == 1, rlk, aux));
    // the outputs: two polynomials of the result's level that are neither each other nor anything the evaluation reads
    std::shared_ptr<Poly> o0 = get<Poly>(out0, T_POLY), o1 = get<Poly>(out1, T_POLY);
    if (!o0 || !o1) return fail(HE_EHANDLE, "%s: bad output handle", who);
    if (plan.out_level < 0) return fail(HE_EINVAL, "%s: the result would sink below level 0", who);
    for (const std::shared_ptr<Poly> &o : {o0, o1}) {
        if (o->ctx != pb->ev->be->ctx || o->N != pb->ev->be->Q->N) return fail(HE_EINVAL, "%s: an output belongs to another context or degree", who);
        if (o->nlimbs < plan.out_level + 1) return fail(HE_EINVAL, "%s: an output has %d limbs, %d needed", who, o->nlimbs, plan.out_level + 1);
        if (o->batch != pb->batch) return fail(HE_EINVAL, "%s: batch mismatch (an output has %d entries, %d expected)", who, o->batch, pb->batch);
    }
    if (o0->d == o1->d) return fail(HE_EINVAL, "%s: the two outputs are the same polynomial", who);
    for (const auto &kv : pb->X)
        for (he_handle xh : kv.second.v) {
            const std::shared_ptr<Poly> x = get<Poly>(xh, T_POLY);
            if (x && (x->d == o0->d || x->d == o1->d)) return fail(HE_EINVAL, "%s: an output is a component of X^{%d}", who, kv.first);
        }
    return polyeval_exec(*pb, plan, 0, scheme == 1, t, rlk, aux, hpoly, p, out0, out1);
}
int he_polyeval_evaluate(he_handle hev, he_handle hpoly, int scheme, uint64_t t, he_handle rlk, int level, he_handle in0, he_handle in1, int n_aux,
                         const int *aux_kind, const uint64_t *aux_s0, const uint64_t *aux_s1, int aux_words, he_handle out0, he_handle out1) {
    static const char *who = "he_polyeval_evaluate";
    GET(p, PolyevalPoly, hpoly, T_POLYEVAL);
    // Evaluate (polynomial_evaluator.go:62-65): the depth check, then the input's copy -- an output may therefore not be the input
    const int depth = p->plan.depth;
    if (level < depth) return fail(HE_EINVAL, "%d levels < %d log(d) -> cannot evaluate poly", level, depth);
    std::shared_ptr<Poly> a = get<Poly>(in0, T_POLY), b = get<Poly>(in1, T_POLY), o0 = get<Poly>(out0, T_POLY), o1 = get<Poly>(out1, T_POLY);
    if (!a || !b || !o0 || !o1) return fail(HE_EHANDLE, "%s: bad Poly handle", who);
    if (o0->d == a->d || o0->d == b->d || o1->d == a->d || o1->d == b->d) return fail(HE_EINVAL, "%s: an output is a component of the input", who);
    if (o0->d == o1->d) return fail(HE_EINVAL, "%s: the two outputs are the same polynomial", who);
    if (o0->nlimbs < p->plan.out_level + 1 || o1->nlimbs < p->plan.out_level + 1) return fail(HE_EINVAL, "%s: an output has too few limbs, %d needed", who, p->plan.out_level + 1);
    if (p->planned_for.size() != 1 || p->planned_for.begin()->second.level != level || p->planned_for.begin()->second.degree != 1)
        return fail(HE_EINVAL, "%s: the polynomial was not planned for a fresh basis at level %d", who, level);
    {   // the refusals of the evaluation itself, before the input is copied
        GET(ev, Evaluator, hev, T_EVAL);
        PolyevalBasis probe;
        probe.ev = ev;
        PolyevalAux aux;
        TRY(polyeval_aux(who, n_aux, aux_kind, aux_s0, aux_s1, aux_words, &aux));
        TRY(polyeval_precheck(who, probe, p->plan, 0, scheme == 1, rlk, aux));
        if (a->batch != o0->batch || a->batch != o1->batch) return fail(HE_EINVAL, "%s: batch mismatch between the input and the outputs", who);
    }
    he_handle hb = 0;
    TRY(he_polyeval_basis_create(hev, polyeval::kMonomial, level, in0, in1, &hb));  // (the plan is the polynomial's: the basis kind is not consulted)
    const int rc = he_polyeval_evaluate_from_power_basis(hb, hpoly, scheme, t, rlk, n_aux, aux_kind, aux_s0, aux_s1, aux_words, out0, out1);
    const std::string msg = g_err;
    he_polyeval_basis_destroy(hb);
    if (rc != HE_OK) g_err = msg;
    return rc;
}
int he_polyeval_gen_power_plan(int basis, int n, int lazy, int n_powers, const int *powers, int64_t *out, size_t cap, size_t *n_words) {
    static const char *who = "he_polyeval_gen_power_plan";
    if (!n_words || (cap && !out)) return fail(HE_EINVAL, "%s: null argument", who);
    if (n < 1) return fail(HE_EINVAL, "invalid n: n=%d should be greater than zero", n);
    if (basis != polyeval::kMonomial && basis != polyeval::kChebyshev) return fail(HE_EINVAL, "%s: unknown basis %d", who, basis);
    polyeval::Plan plan;
    TRY(polyeval_present(who, n_powers, powers, &plan.powers));
    polyeval::gen_power(plan, basis, n, lazy != 0);
    size_t i = 0;
    for (const polyeval::Step &s : plan.steps)
        for (int x : {s.op, s.dst, s.level, s.degree, s.a, s.b}) { if (i < cap) out[i] = x; i++; }
    *n_words = i;
    return HE_OK;
}
int he_polyeval_plan(int degree, int basis, int even, int odd, int lazy, int copy_input, int n_powers, const int *powers, int64_t *out, size_t cap,
                     size_t *n_words) {
    return he_debug_polyeval_plan(degree, basis, even, odd, lazy, copy_input, n_powers, powers, out, cap, n_words);
}
int he_debug_polyeval_plan(int degree, int basis, int even, int odd, int lazy, int copy_input, int n_powers, const int *powers, int64_t *out,
                           size_t cap, size_t *n_words) {
    static const char *who = "he_debug_polyeval_plan";
    if (!n_words || (cap && !out)) return fail(HE_EINVAL, "%s: null argument", who);
    std::map<int, polyeval::Power> present;
    TRY(polyeval_present(who, n_powers, powers, &present));
    const polyeval::Plan p = polyeval::build_plan(degree, basis, even != 0, odd != 0, lazy != 0, present, copy_input != 0);
    if (!p.error.empty()) return fail(HE_EINVAL, "%s", p.error.c_str());
    const std::vector<int64_t> w = polyeval::plan_words(p);
    for (size_t i = 0; i < w.size() && i < cap; i++) out[i] = w[i];
    *n_words = w.size();
    return HE_OK;
}

// the schedule queries of include/hering_debug.h: host only
int he_debug_blindrot_schedule(int logN, const uint64_t *a, int n_lwe, uint64_t *ops, size_t cap, size_t *n_ops) {
    if (!a || !n_ops || n_lwe < 1 || (cap && !ops)) return fail(HE_EINVAL, "he_debug_blindrot_schedule: null argument");
    std::vector<blindrot::Op> l;
    if (!blindrot::blindrot_ops(logN, a, n_lwe, &l))
        return fail(HE_EINVAL, "he_debug_blindrot_schedule: logN out of range, or the row holds a word that is even and not zero, or not below 2N");
    for (size_t i = 0; i < l.size() && i < cap; i++) { ops[2 * i] = (uint64_t)l[i].kind; ops[2 * i + 1] = l[i].arg; }
    *n_ops = l.size();
    return HE_OK;
}
int he_debug_blindrot_rounds(int logN, const uint64_t *a, int batch, int n_lwe, int64_t *rounds, size_t cap, size_t *n_rounds) {
    if (!a || !n_rounds || batch < 1 || n_lwe < 1 || (cap && !rounds)) return fail(HE_EINVAL, "he_debug_blindrot_rounds: null argument");
    std::vector<std::vector<blindrot::Op>> lists((size_t)batch);
    for (int b = 0; b < batch; b++)
        if (!blindrot::blindrot_ops(logN, a + (size_t)b * n_lwe, n_lwe, &lists[(size_t)b]))
            return fail(HE_EINVAL, "he_debug_blindrot_rounds: logN out of range, or row %d holds a word that is even and not zero, or not below 2N", b);
    const std::vector<blindrot::Round> r = blindrot::blindrot_merge(lists);
    for (size_t i = 0; i < r.size() && i < cap; i++)
        for (int b = 0; b < batch; b++) {
            rounds[(2 * i) * (size_t)batch + b] = (int64_t)r[i].gal[(size_t)b];
            rounds[(2 * i + 1) * (size_t)batch + b] = (int64_t)r[i].prod[(size_t)b];
        }
    *n_rounds = r.size();
    return HE_OK;
}

// ---------------------------------------------------------------------------------------
// replayable launch sequences (hipGraph)
// ---------------------------------------------------------------------------------------
int he_graph_begin(he_handle hctx) {
    GET(c, Ctx, hctx, T_CTX);
    // deferred submission: everything ANY thread filed before the capture is launched first -- the dispatcher would otherwise keep
    // launching other threads' earlier requests onto the capturing stream, recording them into the graph instead of running them
    if (c->co->depth.load(std::memory_order_relaxed) > 0) TRY(co_flush_filed(*c));
    Scope sc(c.get());
    if (c->capturing) return fail(HE_EINVAL, "he_graph_begin: the context is already capturing");
    if (prof_active(c->stream)) return fail(HE_EINVAL, "he_graph_begin: kernel profiling is active on this context (he_prof_end first)");
    // relaxed: calls that are not stream work (a pool miss falling through to hipMalloc) stay legal on this thread
    HIP_TRY(hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
    std::lock_guard<std::mutex> lk(c->pool_mu);
    c->capturing = true;
    return HE_OK;
}
int he_graph_end(he_handle hctx, he_handle *out) {
    GET(c, Ctx, hctx, T_CTX);
    if (!out) return fail(HE_EINVAL, "he_graph_end: null output");
    Scope sc(c.get());
    if (!c->capturing) return fail(HE_EINVAL, "he_graph_end: the context is not capturing");
    auto g = std::make_shared<Graph>();
    g->ctx = c;
    {
        std::lock_guard<std::mutex> lk(c->pool_mu);
        c->capturing = false;
        g->hold.swap(c->capture_hold);  // released with the graph, also when the capture failed
    }
    hipGraph_t graph = nullptr;
    hipError_t e = hipStreamEndCapture(c->stream, &graph);
    if (e != hipSuccess || !graph) {
        (void)hipGetLastError();
        return fail(HE_EDEVICE, "he_graph_end: the capture was invalidated (%s): a captured call synchronised, allocated or copied "
                    "from the host", hipGetErrorString(e));
    }
    e = hipGraphInstantiate(&g->exec, graph, nullptr, nullptr, 0);
    size_t nodes = 0;
    (void)hipGraphGetNodes(graph, nullptr, &nodes);
    g->nodes = (int)nodes;
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return fail(HE_EDEVICE, "he_graph_end: hipGraphInstantiate: %s", hipGetErrorString(e));
    c->live_graphs++;  // (under the context lock held by `sc`; released by the graph's destructor, which runs outside any call)
    g->counted = true;
    *out = reg(g);
    return HE_OK;
}
int he_graph_launch(he_handle h) {
    GET(g, Graph, h, T_GRAPH);
    Scope sc(g->ctx.get());
    if (g->ctx->capturing) return fail(HE_EINVAL, "he_graph_launch: the context is capturing");
    HIP_TRY(hipGraphLaunch(g->exec, g->ctx->stream));
    return HE_OK;
}
int he_graph_nodes(he_handle h, int *nodes) {
    GET(g, Graph, h, T_GRAPH);
    if (nodes) *nodes = g->nodes;
    return HE_OK;
}
int he_graph_destroy(he_handle h) { return unreg(h, T_GRAPH); }

// ---------------------------------------------------------------------------------------
// diagnostics
// ---------------------------------------------------------------------------------------
int he_prof_begin(he_handle hctx) {
    GET(c, Ctx, hctx, T_CTX);
    if (c->capturing) return fail(HE_EINVAL, "he_prof_begin: the context is capturing a graph");
    Scope sc(c.get());
    HIP_TRY(hipStreamSynchronize(c->stream));
    prof_begin(c->stream);
    return HE_OK;
}
int he_prof_end(he_handle hctx, int max_kernels, int *counts, float *total_ms, int *n_kernels) {
    GET(c, Ctx, hctx, T_CTX);
    if (!counts || !total_ms || max_kernels < K_COUNT) return fail(HE_EINVAL, "he_prof_end: need room for %d kernels", (int)K_COUNT);
    Scope sc(c.get());
    HIP_TRY(hipStreamSynchronize(c->stream));
    prof_end(c->stream, counts, total_ms);
    if (n_kernels) *n_kernels = K_COUNT;
    return HE_OK;
}
int he_prof_end_bytes(he_handle hctx, int max_kernels, int *counts, float *total_ms, double *total_bytes, int *n_kernels) {
    GET(c, Ctx, hctx, T_CTX);
    if (!counts || !total_ms || !total_bytes || max_kernels < K_COUNT) return fail(HE_EINVAL, "he_prof_end_bytes: need room for %d kernels", (int)K_COUNT);
    Scope sc(c.get());
    HIP_TRY(hipStreamSynchronize(c->stream));
    prof_end(c->stream, counts, total_ms, total_bytes);
    if (n_kernels) *n_kernels = K_COUNT;
    return HE_OK;
}
int he_alg_bytes(he_handle hctx, int reset, double out[2]) {
    GET(c, Ctx, hctx, T_CTX);
    Scope sc(c.get());  // (deferred submission: the calling thread's pending requests are launched -- and accounted -- first)
    if (out) { out[0] = c->alg_bytes[0]; out[1] = c->alg_bytes[1]; }
    if (reset) c->alg_bytes[0] = c->alg_bytes[1] = 0.0;
    return HE_OK;
}
int he_alg_valu(he_handle hctx, int reset, double out[4]) {
    GET(c, Ctx, hctx, T_CTX);
    Scope sc(c.get());
    if (out) for (int i = 0; i < 4; i++) out[i] = c->alg_valu[i];
    if (reset) for (int i = 0; i < 4; i++) c->alg_valu[i] = 0.0;
    return HE_OK;
}
const char *he_prof_kernel_name(int id) { return kernel_name(id); }

int he_probe_modmul(he_handle hctx, int iters, double *out) {
    GET(c, Ctx, hctx, T_CTX);
    if (!out || iters <= 0) return fail(HE_EINVAL, "he_probe_modmul: bad arguments");
    Scope sc(c.get());
    const size_t n = (size_t)1 << 24;
    TRY(c->arena_reserve(n));
    uint64_t *buf = c->arena_take(n);
    HIP_TRY(hipMemsetAsync(buf, 0x5a, n * 8, c->stream));
    const uint64_t q = 0x1fffffffffe00001ull;
    uint64_t inv = q;
    for (int i = 0; i < 6; i++) inv *= 2 - q * inv;
    HIP_TRY(launch_modmul_probe(buf, n, 8, q, inv, c->stream));  // warm-up
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    HIP_TRY(launch_modmul_probe(buf, n, iters, q, inv, c->stream));
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *out = (double)n * iters / (ms * 1e-3);
    return HE_OK;
}

int he_probe_modmul_f64(he_handle hctx, int iters, double *out) {
    GET(c, Ctx, hctx, T_CTX);
    if (!out || iters <= 0) return fail(HE_EINVAL, "he_probe_modmul_f64: bad arguments");
    Scope sc(c.get());
    const size_t n = (size_t)1 << 24;
    TRY(c->arena_reserve(n));
    double *buf = reinterpret_cast<double *>(c->arena_take(n));
    const double q = 35184372744193.0;  // a 45-bit NTT prime of the headline chain
    std::vector<double> h(n);
    for (size_t i = 0; i < n; i++) h[i] = (double)((i * 2654435761ull + 12345ull) % 35184372744193ull);
    HIP_TRY(hipMemcpyAsync(buf, h.data(), n * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(launch_modmul_f64_probe(buf, n, 8, q, c->stream));  // warm-up
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    HIP_TRY(launch_modmul_f64_probe(buf, n, iters, q, c->stream));
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *out = (double)n * iters / (ms * 1e-3);
    return HE_OK;
}

// the scalar primitives one by one (hering_debug.h): tuples up, one launch of the probe kernel, results down
int he_debug_arith(he_handle hring, int limb, int op, size_t n, const uint64_t *a, const uint64_t *b, const uint64_t *c,
                   uint64_t *out0, uint64_t *out1) {
    GET(r, Ring, hring, T_RING);
    static_assert((int)HE_ARITH_COUNT == (int)ARITH_COUNT && (int)HE_ARITH_AUTO_DEST == (int)ARITH_AUTO_DEST, "he_arith_op numbering");
    if (op < 0 || op >= HE_ARITH_COUNT) return fail(HE_EINVAL, "he_debug_arith: unknown op %d", op);
    if (limb < 0 || limb >= r->nmod()) return fail(HE_EINVAL, "he_debug_arith: limb %d out of range", limb);
    if (n == 0 || n > ((size_t)1 << 20)) return fail(HE_EINVAL, "he_debug_arith: n must be in 1 .. 2^20");
    const bool three = (op >= HE_ARITH_BFLY_FWD && op <= HE_ARITH_BFLY_INV_SCALED_ASM) || op == HE_ARITH_AUTO_DEST;
    const bool two = three || op <= HE_ARITH_MRED128_LAZY || op == HE_ARITH_BRED_LAZY || op == HE_ARITH_BRED || op == HE_ARITH_MODMUL_F64;
    const bool pair = three && op != HE_ARITH_AUTO_DEST;
    if (!a || !out0 || (two && !b) || (three && !c) || (pair && !out1)) return fail(HE_EINVAL, "he_debug_arith: op %d misses an array", op);
    Scope sc(r->ctx.get());
    const size_t w = (n + 1) & ~(size_t)1;
    TRY(r->ctx->arena_reserve(5 * w));
    uint64_t *d[5];
    for (int k = 0; k < 5; k++) d[k] = r->ctx->arena_take(n);
    hipStream_t st = r->ctx->stream;
    HIP_TRY(hipMemcpyAsync(d[0], a, n * 8, hipMemcpyHostToDevice, st));
    if (two) HIP_TRY(hipMemcpyAsync(d[1], b, n * 8, hipMemcpyHostToDevice, st));
    if (three) HIP_TRY(hipMemcpyAsync(d[2], c, n * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(launch_arith_probe(r->d_mc + limb, op, n, d[0], two ? d[1] : nullptr, three ? d[2] : nullptr, d[3], pair ? d[4] : nullptr, st));
    HIP_TRY(hipMemcpyAsync(out0, d[3], n * 8, hipMemcpyDeviceToHost, st));
    if (pair) HIP_TRY(hipMemcpyAsync(out1, d[4], n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return HE_OK;
}

// ---------------------------------------------------------------------------------------
// RCCL over xGMI ("RCCL only for key distribution", and the partial accumulators of a key switch split
// over the GPUs by digit).  librccl is loaded at run time and driven directly on the context's stream: no framework in the
// data path and no second HIP runtime in the process (librccl.so.1 binds to the libamdhip64 this library already uses).
// ---------------------------------------------------------------------------------------
extern "C++" {
namespace {
typedef struct ncclComm *rccl_comm_t;
typedef struct { char internal[128]; } rccl_id_t;
constexpr int kRcclUint64 = 5, kRcclSum = 0;  // ncclDataType_t / ncclRedOp_t of rccl.h
struct RcclApi {
    void *so = nullptr;
    int (*GetUniqueId)(rccl_id_t *) = nullptr;
    int (*CommInitRank)(rccl_comm_t *, int, rccl_id_t, int) = nullptr;
    int (*CommDestroy)(rccl_comm_t) = nullptr;
    int (*Broadcast)(const void *, void *, size_t, int, int, rccl_comm_t, hipStream_t) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, rccl_comm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    std::string why, path;
};
RcclApi &rccl() {
    static RcclApi api = [] {
        RcclApi a;
        // first choice: the librccl that sits next to the HIP runtime this process actually loaded (a framework imported before
        // this library brings its own pair -- torch/lib/libamdhip64.so + librccl.so -- and an RCCL build should meet the runtime
        // it was built with); then the system's
        std::vector<std::string> names;
        Dl_info info;
        if (dladdr((void *)&hipGetDeviceCount, &info) && info.dli_fname) {
            std::string dir(info.dli_fname);
            const size_t slash = dir.rfind('/');
            if (slash != std::string::npos) {
                dir.resize(slash);
                names.push_back(dir + "/librccl.so.1");
                names.push_back(dir + "/librccl.so");
            }
        }
        for (const char *n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) names.push_back(n);
        for (const std::string &name : names) {
            a.so = dlopen(name.c_str(), RTLD_NOW | RTLD_LOCAL);
            if (a.so) { a.path = name; break; }
        }
        if (!a.so) { a.why = dlerror() ? dlerror() : "librccl.so.1 not found"; return a; }
        auto sym = [&](const char *n) { void *p = dlsym(a.so, n); if (!p) a.why = std::string("missing symbol ") + n; return p; };
        a.GetUniqueId = (decltype(a.GetUniqueId))sym("ncclGetUniqueId");
        a.CommInitRank = (decltype(a.CommInitRank))sym("ncclCommInitRank");
        a.CommDestroy = (decltype(a.CommDestroy))sym("ncclCommDestroy");
        a.Broadcast = (decltype(a.Broadcast))sym("ncclBroadcast");
        a.AllReduce = (decltype(a.AllReduce))sym("ncclAllReduce");
        a.GetErrorString = (decltype(a.GetErrorString))sym("ncclGetErrorString");
        return a;
    }();
    return api;
}
int rccl_ready() {
    RcclApi &a = rccl();
    if (!a.so || !a.why.empty()) return fail(HE_EDEVICE, "RCCL is not available: %s", a.why.c_str());
    return HE_OK;
}
#define RCCL_TRY(expr)                                                                                                  \
    do {                                                                                                                \
        int _r = (expr);                                                                                                \
        if (_r != 0) return fail(HE_EDEVICE, "%s: %s", #expr, rccl().GetErrorString ? rccl().GetErrorString(_r) : "?"); \
    } while (0)
struct Comm : Obj {
    std::shared_ptr<Ctx> ctx;
    rccl_comm_t comm = nullptr;
    int rank = 0, world = 0;
    Comm() : Obj(T_COMM) {}
    ~Comm() override {
        hipSetDevice(ctx->dev);
        hipStreamSynchronize(ctx->stream);
        if (comm) rccl().CommDestroy(comm);
    }
};
}  // namespace
}  // extern "C++"
int he_rccl_available(int *yes) {
    if (!yes) return fail(HE_EINVAL, "he_rccl_available: null output");
    RcclApi &a = rccl();
    *yes = (a.so && a.why.empty()) ? 1 : 0;
    return HE_OK;
}
int he_rccl_unique_id(uint8_t *id) {
    if (!id) return fail(HE_EINVAL, "he_rccl_unique_id: null output");
    TRY(rccl_ready());
    rccl_id_t u;
    RCCL_TRY(rccl().GetUniqueId(&u));
    memcpy(id, u.internal, sizeof u.internal);
    return HE_OK;
}
int he_rccl_comm_create(he_handle hctx, const uint8_t *id, int rank, int world, he_handle *out) {
    GET(c, Ctx, hctx, T_CTX);
    if (!id || !out || world <= 0 || rank < 0 || rank >= world) return fail(HE_EINVAL, "he_rccl_comm_create: bad arguments");
    TRY(rccl_ready());
    auto m = std::make_shared<Comm>();
    m->ctx = c; m->rank = rank; m->world = world;
    rccl_id_t u;
    memcpy(u.internal, id, sizeof u.internal);
    // The communicator is bound to the device current at the call; the context's lock is NOT held across the rendezvous: a peer
    // that never arrives must cost the caller this thread (lattigo_amd/dist.py gives it a deadline), not every later call on the
    // context.
    HIP_TRY(hipSetDevice(c->dev));
    RCCL_TRY(rccl().CommInitRank(&m->comm, world, u, rank));
    *out = reg(m);
    return HE_OK;
}
int he_rccl_comm_destroy(he_handle h) { return unreg(h, T_COMM); }
int he_rccl_comm_ranks(he_handle h, int *ranks) {
    GET(m, Comm, h, T_COMM);
    if (!ranks) return fail(HE_EINVAL, "he_rccl_comm_ranks: null output");
    Ctx *c = m->ctx.get();
    Scope sc(c);
    TRY(c->arena_reserve(2));
    uint64_t *d = c->arena_take(2), one = 1, sum = 0;
    HIP_TRY(hipMemcpyAsync(d, &one, 8, hipMemcpyHostToDevice, c->stream));
    RCCL_TRY(rccl().AllReduce(d, d, 1, kRcclUint64, kRcclSum, m->comm, c->stream));
    HIP_TRY(hipMemcpyAsync(&sum, d, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *ranks = (int)sum;
    return HE_OK;
}
int he_evk_broadcast(he_handle hcomm, he_handle hk, int root) {
    GET(m, Comm, hcomm, T_COMM);
    GET(k, Evk, hk, T_EVK);
    Ctx *c = m->ctx.get();
    if (k->ev->be->ctx.get() != c) return fail(HE_EINVAL, "he_evk_broadcast: the key belongs to another context than the communicator");
    if (root < 0 || root >= m->world) return fail(HE_EINVAL, "he_evk_broadcast: root %d outside [0, %d)", root, m->world);
    Scope sc(c);
    const size_t words = (size_t)k->beta * 2 * (size_t)(k->nQk + k->nPk) * k->ev->be->Q->N;
    RCCL_TRY(rccl().Broadcast(k->d, k->d, words, kRcclUint64, root, m->comm, c->stream));
    if (m->rank != root) TRY(evk_derive(*k));  // the derived double-precision copy follows the new words (same stream: ordered)
    return HE_OK;
}
int he_poly_all_reduce_sum(he_handle hcomm, he_handle hp) {
    GET(m, Comm, hcomm, T_COMM);
    GET(p, Poly, hp, T_POLY);
    Ctx *c = m->ctx.get();
    if (p->ctx.get() != c) return fail(HE_EINVAL, "he_poly_all_reduce_sum: the polynomial belongs to another context than the communicator");
    Scope sc(c);
    RCCL_TRY(rccl().AllReduce(p->d, p->d, (size_t)p->batch * p->nlimbs * p->N, kRcclUint64, kRcclSum, m->comm, c->stream));
    return HE_OK;
}

// concurrent single-ciphertext callers (hering_debug.h): the measurement harness of bench.py's `concurrent_b1`
namespace {
struct ConcArg {
    int idx, iters, sync_each, bgv, level;
    uint64_t t;
    he_handle ctx, eval, a0, a1, b0, b1, rlk, o0, o1;
    std::atomic<int> *go;  // 0: wait, 1: run, -1: give up (a thread could not be started)
    double t0, t1;
    int rc;
    std::string err;
};
double mono_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
void *conc_worker(void *vp) {
    ConcArg &a = *(ConcArg *)vp;
    int g;
    while ((g = a.go->load(std::memory_order_acquire)) == 0) sched_yield();
    if (g < 0) return nullptr;
    a.t0 = mono_s();
    for (int i = 0; i < a.iters && a.rc == 0; i++) {
        switch (a.bgv) {  // (the operation selector of he_debug_concurrent_mul_relin)
            case 0: a.rc = he_ckks_mul_relin(a.eval, a.level, a.a0, a.a1, a.b0, a.b1, a.rlk, a.o0, a.o1, 0); break;
            case 1: a.rc = he_bgv_mul_relin(a.eval, a.level, a.t, a.a0, a.a1, a.b0, a.b1, a.rlk, a.o0, a.o1, 0); break;
            case 2: a.rc = he_automorphism_ct(a.eval, a.level, a.a0, a.a1, a.t, a.rlk, a.o0, a.o1); break;
            case 3: a.rc = he_relinearize(a.eval, a.level, a.a0, a.a1, a.b0, a.rlk, a.o0, a.o1); break;
            default: a.rc = he_gadget_product(a.eval, a.level, a.a0, a.rlk, a.o0, a.o1); break;
        }
        if (a.rc == 0 && a.sync_each) a.rc = he_ctx_sync(a.ctx);
    }
    if (a.rc == 0) a.rc = he_ctx_sync(a.ctx);
    if (a.rc != 0) a.err = g_err;
    a.t1 = mono_s();
    return nullptr;
}
}  // namespace
int he_debug_concurrent_mul_relin(int n_threads, int iters, int sync_each, int bgv, int level, uint64_t t, const he_handle *ctx,
                                  const he_handle *eval, const he_handle *a0, const he_handle *a1, const he_handle *b0,
                                  const he_handle *b1, const he_handle *rlk, const he_handle *o0, const he_handle *o1,
                                  double *wall_s) {
    if (n_threads <= 0 || n_threads > 4096 || iters <= 0 || !ctx || !eval || !a0 || !a1 || !b0 || !b1 || !rlk || !o0 || !o1 || !wall_s ||
        bgv < 0 || bgv > 4)
        return fail(HE_EINVAL, "he_debug_concurrent_mul_relin: bad arguments");
    std::vector<ConcArg> args(n_threads);
    std::vector<pthread_t> th(n_threads);
    // all threads or none: they wait for `go`, which says "run" only once every one of them exists (a barrier sized for threads
    // that were never created would not open, and joining handles that were never filled is undefined)
    std::atomic<int> go{0};
    int started = 0;
    for (int i = 0; i < n_threads; i++) {
        args[i] = ConcArg{i, iters, sync_each, bgv, level, t, ctx[i], eval[i], a0[i], a1[i], b0[i], b1[i], rlk[i], o0[i], o1[i], &go, 0, 0, 0, {}};
        if (pthread_create(&th[i], nullptr, conc_worker, &args[i]) != 0) break;
        started++;
    }
    go.store(started == n_threads ? 1 : -1, std::memory_order_release);
    for (int i = 0; i < started; i++) pthread_join(th[i], nullptr);
    if (started != n_threads) return fail(HE_ENOMEM, "he_debug_concurrent_mul_relin: could not start %d threads", n_threads);
    double lo = args[0].t0, hi = args[0].t1;
    for (const ConcArg &a : args) { lo = std::min(lo, a.t0); hi = std::max(hi, a.t1); }
    *wall_s = hi - lo;
    for (const ConcArg &a : args)
        if (a.rc != 0) return fail(a.rc, "thread %d: %s", a.idx, a.err.c_str());
    return HE_OK;
}

}  // extern "C"
