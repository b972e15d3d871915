// fpe_engine.cpp — the C ABI of include/fpe.h over the gfx950 kernels (fpe_kernels.hip).
// Owns device memory: immutable map snapshots (swapped atomically, so a plan keeps the snapshot it
// started with — the reference races on gridmap_, cpp:506 vs cpp:818) and the spiral rank table.
// There is NO CPU compute path: without a usable GPU every compute entry point fails.
#include <hip/hip_runtime.h>
#include <chrono>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <condition_variable>
#include <deque>
#include <limits>
#include <thread>
#include <type_traits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "fpe_host.hpp"
#include "fpe_launch.hpp"

namespace {

thread_local std::string g_err;
thread_local fpe_service_gate g_gate = {255, FPE_GATE_NONE, 0, 0, {0, 0, 0, 0}, 0.0, 0.0};  // verdict of this thread's last fpe_plan_service* call
thread_local const void* g_gateEngine = nullptr;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int fail_hip(hipError_t e, const char* what) {
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    return FPE_E_HIP;
}
#define FPE_HIP(call)                                     \
    do {                                                  \
        hipError_t e_ = (call);                           \
        if (e_ != hipSuccess) return fail_hip(e_, #call); \
    } while (0)

// Layer buffers of retired snapshots are recycled instead of freed: a traversability map arrives
// at 10-20 Hz and hipMalloc/hipFree (the latter a device-wide sync) would dominate the upload.
// Lifetime without per-launch GPU work: a snapshot retired while device-API (asynchronous) launches may still
// read it hands its buffers over marked "dirty"; whoever takes a dirty buffer — an upload or a bit-plane build,
// 10-20 Hz paths — synchronises the device once before writing it.  Plans never pay for this: an event recorded
// after every launch would put a 3-4 us bubble between back-to-back plan kernels (measured).
struct BufferPool {
    struct Entry {
        size_t n;      // capacity in 4-byte units
        float* p;
        bool dirty;    // retired while asynchronous (device-API) work may still have been reading it
    };
    std::mutex mu;
    std::vector<Entry> free;
    // Best fit: the smallest pooled buffer that holds n units and is not more than twice as large (a map stream whose
    // size changes from message to message keeps recycling instead of falling back to hipMalloc / hipFree, which
    // synchronise the device).  *cap receives the buffer's real capacity: the caller hands THAT back to give().
    // cleanOnly: skip buffers that need a device synchronisation before reuse (the plan path never pays for one).
    float* take(size_t n, bool* dirty, size_t* cap, bool cleanOnly = false) {
        std::lock_guard<std::mutex> lk(mu);
        size_t best = free.size();
        for (size_t k = 0; k < free.size(); ++k) {
            if (free[k].n < n || free[k].n > 2 * n + 1024) continue;
            if (cleanOnly && free[k].dirty) continue;
            if (best == free.size() || free[k].n < free[best].n) best = k;
        }
        if (best == free.size()) {
            *dirty = false;
            *cap = 0;
            return nullptr;
        }
        float* p = free[best].p;
        *dirty = free[best].dirty;
        *cap = free[best].n;
        free.erase(free.begin() + static_cast<long>(best));
        return p;
    }
    void give(size_t n, float* p, bool dirty = false) {
        float* drop = nullptr;
        {
            std::lock_guard<std::mutex> lk(mu);
            if (free.size() >= 12) {  // two snapshots' worth (layers + bit planes) plus the upload staging layer
                drop = free.front().p;
                free.erase(free.begin());
            }
            free.push_back(Entry{n, p, dirty});
        }
        if (drop) (void)hipFree(drop);  // hipFree synchronises the device: safe for a dirty buffer too
    }
    ~BufferPool() {
        for (auto& e : free) (void)hipFree(e.p);
    }
};

// Per-call resources of the host-buffer entry points (stream, one device arena, one pinned host
// arena), recycled across calls: a plan_global_footholds call must not pay for hipMalloc /
// hipStreamCreate (3.6 ms per call before this pool, ~0.1 ms after).  Concurrent calls each take
// their own context.
struct CallCtx {
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr;  // the opt track's chain of a small plan + opt call runs beside the plan kernel (plan_host)
    unsigned char* dev = nullptr;
    size_t devCap = 0;
    unsigned char* pinned = nullptr;
    size_t pinCap = 0;
    std::vector<hipEvent_t> events;  // one per staged result chunk in flight (created on demand, kept)
    // work may be queued on `stream` that reads / writes the arenas (and the caller's pinned arrays): set before the first
    // enqueue of a call, cleared once the call has synchronised.  A call that leaves early (a failed HIP call after its
    // kernels were queued) hands the context back with the flag set, and the lease waits for the stream before the next
    // call's memcpy can touch the arena the kernels are still reading.
    bool inFlight = false;
    uint32_t doneSeq = 0;  // sequence number of the completion word of polled one-pose calls (plan_host)
    ~CallCtx() {
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        if (dev) (void)hipFree(dev);
        if (pinned) (void)hipHostFree(pinned);
        if (stream) (void)hipStreamDestroy(stream);
        if (side) (void)hipStreamDestroy(side);
    }
    hipError_t side_stream(hipStream_t* out) {
        if (!side) {
            // highest priority: the chain is the call's critical path — and a priority stream gets a hardware queue of its own class,
            // where a second default-priority stream may land on the SAME queue as `stream` (the runtime spreads a process's streams
            // over a few hardware queues) and run behind the plan kernel: measured in bench.py's process, many streams alive, as
            // 150 us per service call against 138 with the kernels one after the other and 105 in a process of its own
            int lo = 0, hi = 0;
            hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);
            if (e == hipSuccess) e = hipStreamCreateWithPriority(&side, hipStreamNonBlocking, hi);
            if (e != hipSuccess) {  // (no priorities on this runtime: a plain stream — correct, possibly behind the plan kernel)
                (void)hipGetLastError();
                side = nullptr;
                e = hipStreamCreateWithFlags(&side, hipStreamNonBlocking);
                if (e != hipSuccess) return e;
            }
        }
        *out = side;
        return hipSuccess;
    }
    hipError_t event(size_t k, hipEvent_t* out) {
        while (events.size() <= k) {
            hipEvent_t e = nullptr;
            hipError_t rc = hipEventCreateWithFlags(&e, hipEventDisableTiming);
            if (rc != hipSuccess) return rc;
            events.push_back(e);
        }
        *out = events[k];
        return hipSuccess;
    }
    hipError_t reserve(size_t bytes) {
        if (!stream) {
            hipError_t e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
            if (e != hipSuccess) return e;
        }
        if (bytes > devCap) {
            if (dev) (void)hipFree(dev);
            dev = nullptr;
            devCap = 0;
            const size_t cap = std::max<size_t>(bytes + bytes / 4, 1 << 16);
            hipError_t e = hipMalloc(reinterpret_cast<void**>(&dev), cap);
            if (e != hipSuccess) return e;
            devCap = cap;
        }
        if (bytes > pinCap) {
            if (pinned) (void)hipHostFree(pinned);
            pinned = nullptr;
            pinCap = 0;
            const size_t cap = std::max<size_t>(bytes + bytes / 4, 1 << 16);
            hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&pinned), cap, hipHostMallocDefault);
            if (e != hipSuccess) return e;
            pinCap = cap;
        }
        return hipSuccess;
    }
};
struct CtxPool {
    std::mutex mu;
    std::vector<std::unique_ptr<CallCtx>> free;
    std::unique_ptr<CallCtx> take() {
        std::lock_guard<std::mutex> lk(mu);
        if (free.empty()) return std::unique_ptr<CallCtx>(new CallCtx());
        std::unique_ptr<CallCtx> c = std::move(free.back());
        free.pop_back();
        return c;
    }
    void give(std::unique_ptr<CallCtx> c) {
        std::lock_guard<std::mutex> lk(mu);
        if (free.size() < 8) free.push_back(std::move(c));
    }
};
struct CtxLease {  // returns the context to the pool on every exit path
    CtxPool& pool;
    std::unique_ptr<CallCtx> ctx;
    explicit CtxLease(CtxPool& p) : pool(p), ctx(p.take()) {}
    ~CtxLease() {
        if (ctx && ctx->inFlight && ctx->stream) {
            (void)hipStreamSynchronize(ctx->stream);  // best effort: an early exit after work was queued
            if (ctx->side) (void)hipStreamSynchronize(ctx->side);
            ctx->inFlight = false;
        }
        pool.give(std::move(ctx));
    }
};
inline size_t align256(size_t n) { return (n + 255) & ~static_cast<size_t>(255); }

// Copy-out of large results from the pinned arena into the caller's (pageable) arrays: a few persistent host threads,
// so that the copy of chunk k runs while chunk k+1 is still crossing PCIe (one thread moves ~25 GB/s, the link ~50).
class CopyPool {
  public:
    ~CopyPool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : threads_) t.join();
    }
    struct Batch {
        std::mutex mu;
        std::condition_variable cv;
        int pending = 0;
    };
    void submit(Batch& b, void* dst, const void* src, size_t len) {
        {
            std::lock_guard<std::mutex> lk(b.mu);
            ++b.pending;
        }
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (threads_.empty()) start();
            q_.push_back(Task{&b, dst, src, len});
        }
        cv_.notify_one();
    }
    static void wait(Batch& b) {
        std::unique_lock<std::mutex> lk(b.mu);
        b.cv.wait(lk, [&] { return b.pending == 0; });
    }
    static size_t width() {  // threads of the pool (start())
        const unsigned n = std::thread::hardware_concurrency();
        return n > 4 ? 3 : (n > 1 ? n - 1 : 1);
    }

  private:
    struct Task {
        Batch* b;
        void* dst;
        const void* src;
        size_t len;
    };
    void start() {  // under mu_
        const size_t n = width();
        for (size_t k = 0; k < n; ++k) threads_.emplace_back([this] { run(); });
    }
    void run() {
        for (;;) {
            Task t;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
                if (q_.empty()) return;
                t = q_.front();
                q_.pop_front();
            }
            std::memcpy(t.dst, t.src, t.len);
            {
                std::lock_guard<std::mutex> lk(t.b->mu);
                if (--t.b->pending == 0) t.b->cv.notify_all();
            }
        }
    }
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<Task> q_;
    std::vector<std::thread> threads_;
    bool stop_ = false;
};

// Is `p` host memory the GPU can write by DMA (hipHostMalloc / hipHostRegister / fpe_host_alloc)?  Then results are
// copied from the device straight into it.
bool is_pinned_host(const void* p) {
    hipPointerAttribute_t a;
    std::memset(&a, 0, sizeof(a));
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // an ordinary malloc'ed pointer is reported as an error: not sticky
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// Bit planes of a snapshot for one (defaultFootholdThreshold, candidateFootholdThreshold) pair: built by the upload
// for the pairs the previous snapshot was planned with (the upload already owns the pool's synchronisation), lazily by
// the first plan for a pair never seen before.  Shared: a call keeps the set it launched with alive, so the snapshot
// can evict its least recently used set when a fifth pair arrives (no silent change of kernels).
struct MaskSet {
    float thrD = 0.0f, thrC = 0.0f;
    uint32_t* d_words = nullptr;
    size_t cap = 0;  // capacity in 4-byte units (what goes back to the pool)
    int strideW = 0, nw = 0;
    hipEvent_t ready = nullptr;
    std::atomic<bool> readyDone{false};
    std::atomic<bool> asyncUsed{false};
    std::atomic<unsigned long long> lastUse{0};
    std::shared_ptr<BufferPool> pool;
    ~MaskSet() {
        if (ready) {
            (void)hipEventSynchronize(ready);
            (void)hipEventDestroy(ready);
        }
        if (d_words) pool ? pool->give(cap, reinterpret_cast<float*>(d_words), asyncUsed.load(std::memory_order_acquire)) : (void)hipFree(d_words);
    }
};

struct MapSnapshot {
    fpe::MapGeom g;
    size_t n = 0;
    size_t capTrav = 0, capElev = 0;  // pooled capacities of the two layers
    float* d_trav = nullptr;
    float* d_elev = nullptr;
    std::shared_ptr<BufferPool> pool;
    // `ready` is recorded on the uploading stream after the copy / canonicalise work; a consumer stream waits on
    // it before its first kernel until the event has been seen complete once (then no GPU-side wait is queued
    // any more).  `asyncUsed`: some device-API launch read this snapshot without the host waiting for it.
    hipEvent_t ready = nullptr;
    std::atomic<bool> readyDone{false};
    std::atomic<bool> asyncUsed{false};
    std::mutex mu;
    std::vector<std::shared_ptr<MaskSet>> masks;
    unsigned long long useClock = 0;  // guarded by mu

    hipError_t wait_ready(hipStream_t s) {
        if (!ready || readyDone.load(std::memory_order_acquire)) return hipSuccess;
        if (hipEventQuery(ready) == hipSuccess) {
            readyDone.store(true, std::memory_order_release);
            return hipSuccess;
        }
        return hipStreamWaitEvent(s, ready, 0);
    }
    void note_async_use() { asyncUsed.store(true, std::memory_order_release); }
    ~MapSnapshot() {
        const bool dirty = asyncUsed.load(std::memory_order_acquire);
        if (ready) {
            (void)hipEventSynchronize(ready);  // the upload itself (normally long complete)
            (void)hipEventDestroy(ready);
        }
        for (auto& ms : masks)
            if (dirty) ms->asyncUsed.store(true, std::memory_order_release);
        masks.clear();
        if (d_trav) pool ? pool->give(capTrav, d_trav, dirty) : (void)hipFree(d_trav);
        if (d_elev) pool ? pool->give(capElev, d_elev, dirty) : (void)hipFree(d_elev);
    }
};

constexpr size_t kMaxLdsBytes = 160 * 1024;
constexpr size_t kLayerPadBytes = 128;  // >= kRowOverreadBytes of fpe_kernels.hip (96)
constexpr size_t kZeroCopyBytes = 64 * 1024;  // fpe_plan calls up to this size run on the pinned arena directly

}  // namespace

struct fpe_engine {
    int device = 0;
    std::mutex mu;
    std::mutex updateMu;  // fpe_update_map*: updates of one engine serialise among themselves (each takes the snapshot current at entry as its base)
    std::shared_ptr<MapSnapshot> map;
    std::shared_ptr<BufferPool> pool = std::make_shared<BufferPool>();
    CtxPool ctxPool;
    CopyPool copyPool;
    int16_t* d_di = nullptr;
    int16_t* d_dj = nullptr;
    uint8_t* d_ring = nullptr;
    int32_t* d_ringStart = nullptr;
    uint32_t* d_packed = nullptr;
    uint32_t* d_fast16 = nullptr;
    int maxRing = 0;
    std::vector<int32_t> ringStart;   // host copy of the rank table's ring offsets
    float maxLegSearchRadius = 0.0f;  // fpe_set_max_leg_search_radius
    fpe::Tuning tuning;               // fpe_set_tuning; seeded from the environment once, in fpe_create
    // The traversability-only filter chain's step_height scratch: up to kFilterSlots buffers, each with the event recorded behind
    // the last chain that used it.  A chain takes, in this order: the buffer its own stream used last (chains of one stream run in
    // order: nothing to wait for — a 10-20 Hz producer on its own stream never waits and never synchronises), a buffer whose last
    // chain has completed (neither when it is more than four times too large: a single huge map must not pin memory for good), a fresh buffer while there are free slots, and only then the least recently used busy buffer, behind
    // a GPU-side hipStreamWaitEvent on its event.  No path synchronises the device or blocks the host (round 5 kept ONE buffer
    // keyed to one stream: two producers alternating streams paid a hipDeviceSynchronize per call).
    // A stream handed to fpe_traversability_device must outlive the chains queued on it (include/fpe.h).
    static constexpr int kFilterSlots = 4;
    struct FilterSlot {
        float* buf = nullptr;
        size_t cap = 0;
        hipEvent_t done = nullptr;
        hipStream_t last = nullptr;
        unsigned long long use = 0;
    };
    std::mutex filterMu;
    FilterSlot filterSlots[kFilterSlots];
    unsigned long long filterClock = 0;

    fpe::SpiralLut lut() const {
        return fpe::SpiralLut{d_di, d_dj, d_ring, d_ringStart, maxRing, ringStart.empty() ? 0 : ringStart[static_cast<size_t>(maxRing) + 1], d_packed, d_fast16};
    }
};

namespace {

// Device allocation in 4-byte units with the tail padding every pooled buffer carries (the row scan reads whole
// 16-byte groups past the end of a layer, fpe_kernels.hip::rows_issue), so any pooled buffer can serve any role.
// *cap: the capacity to hand back to the pool.  cleanOnly: never synchronise the device (the plan path).
hipError_t alloc_units(BufferPool& pool, size_t n, float** out, size_t* cap, bool cleanOnly = false) {
    bool dirty = false;
    *out = pool.take(n, &dirty, cap, cleanOnly);
    if (*out) return dirty ? hipDeviceSynchronize() : hipSuccess;  // see BufferPool: asynchronous readers may be in flight
    *cap = n;
    return hipMalloc(reinterpret_cast<void**>(out), n * sizeof(float) + kLayerPadBytes);
}
// One pooled buffer of a call, returned to the pool on every exit path: recycled like the snapshot layers (a 10-20 Hz map stream
// must not hipMalloc / hipFree per message).  dirty: work queued on it may still run when the call returns — its next taker
// synchronises the device before reuse (BufferPool).
struct PooledBuf {
    std::shared_ptr<BufferPool> pool;
    bool dirty;
    size_t cap = 0;
    float* p = nullptr;
    hipError_t take(size_t n, bool cleanOnly = false) { return alloc_units(*pool, n, &p, &cap, cleanOnly); }
    ~PooledBuf() {
        if (p) pool->give(cap, p, dirty);
    }
};

// What one launch needs besides the constants: the snapshot, and (bit-window path) its bit planes.
struct CallPlan {
    std::shared_ptr<MapSnapshot> snap;
    fpe::PlanConsts pc;
    size_t planLds = 0, searchLds = 0;
    bool useBits = false;
    fpe::BitMap bits{nullptr, 0, 0};
    std::shared_ptr<MaskSet> mask;  // the bit planes this call launches with (kept alive past an eviction)
};

// Bit planes of `snap` for a threshold pair: queued on `stream`, event recorded.  cleanOnly as in alloc_units.
// fill false: the buffer only — the caller's canonicalising kernel writes the planes while the layer passes through it
// (launch_canonicalise with d_planeWords) and then calls mask_ready.
int alloc_mask(MapSnapshot& snap, float thrD, float thrC, bool cleanOnly, std::shared_ptr<MaskSet>& out) {
    auto ms = std::make_shared<MaskSet>();
    ms->thrD = thrD;
    ms->thrC = thrC;
    ms->pool = snap.pool;
    const size_t need = fpe::bitmap_words(snap.g.rows, snap.g.cols, &ms->strideW, &ms->nw);
    float* buf = nullptr;
    FPE_HIP(alloc_units(*snap.pool, need, &buf, &ms->cap, cleanOnly));
    ms->d_words = reinterpret_cast<uint32_t*>(buf);
    out = std::move(ms);
    return FPE_OK;
}
int mask_ready(MaskSet& ms, hipStream_t stream) {
    hipError_t e = hipEventCreateWithFlags(&ms.ready, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(ms.ready, stream);
    if (e != hipSuccess) {
        ms.asyncUsed.store(true);  // the build may be queued: hand the buffer back dirty
        return fail_hip(e, "bit-plane build");
    }
    return FPE_OK;
}
int build_mask(MapSnapshot& snap, float thrD, float thrC, hipStream_t stream, bool cleanOnly, std::shared_ptr<MaskSet>& out) {
    std::shared_ptr<MaskSet> ms;
    const int rc0 = alloc_mask(snap, thrD, thrC, cleanOnly, ms);
    if (rc0 != FPE_OK) return rc0;
    hipError_t e = fpe::launch_build_bitmap(snap.d_trav, snap.g.rows, snap.g.cols, thrD, thrC, ms->d_words, stream);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ms->ready, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(ms->ready, stream);
    if (e != hipSuccess) {
        ms->asyncUsed.store(true);  // the build may be queued: hand the buffer back dirty
        return fail_hip(e, "bit-plane build");
    }
    out = std::move(ms);
    return FPE_OK;
}
// The planes of the carried pairs from `first` on, from the new snapshot's finished traversability layer, behind `stream`.
int build_carried_planes(MapSnapshot& snap, const std::vector<std::pair<float, float>>& pairs, size_t first, hipStream_t stream, bool cleanOnly) {
    for (size_t k = first; k < pairs.size(); ++k) {
        std::shared_ptr<MaskSet> ms;
        const int rc = build_mask(snap, pairs[k].first, pairs[k].second, stream, cleanOnly, ms);
        if (rc != FPE_OK) return rc;
        ms->lastUse.store(++snap.useClock);
        snap.masks.push_back(std::move(ms));
    }
    return FPE_OK;
}

// The snapshot's bit planes for a threshold pair into cp.mask / cp.bits, `stream` ordered after their build.  A pair this snapshot
// has not been planned with (the upload pre-builds the pairs of the previous snapshot) is built here on `stream`, into fresh memory
// when no clean pooled buffer is free (a call never synchronises the device for a recycled buffer); a fifth pair evicts the least
// recently used set (calls in flight keep theirs alive).
int acquire_mask(MapSnapshot& snap, float thrD, float thrC, hipStream_t stream, CallPlan& cp) {
    std::lock_guard<std::mutex> lk(snap.mu);
    std::shared_ptr<MaskSet> found;
    for (auto& ms : snap.masks)
        if (std::memcmp(&ms->thrD, &thrD, 4) == 0 && std::memcmp(&ms->thrC, &thrC, 4) == 0) found = ms;
    if (!found) {
        const int rc = build_mask(snap, thrD, thrC, stream, true, found);
        if (rc != FPE_OK) return rc;
        if (snap.masks.size() >= 4) {
            size_t lru = 0;
            for (size_t k = 1; k < snap.masks.size(); ++k)
                if (snap.masks[k]->lastUse.load() < snap.masks[lru]->lastUse.load()) lru = k;
            if (snap.asyncUsed.load(std::memory_order_acquire)) snap.masks[lru]->asyncUsed.store(true);
            snap.masks.erase(snap.masks.begin() + static_cast<long>(lru));
        }
        snap.masks.push_back(found);
    }
    found->lastUse.store(++snap.useClock);
    cp.mask = found;
    cp.bits = fpe::BitMap{reinterpret_cast<const uint4*>(found->d_words), found->strideW, found->nw};
    if (!found->readyDone.load(std::memory_order_acquire)) {
        if (hipEventQuery(found->ready) == hipSuccess) found->readyDone.store(true, std::memory_order_release);
        else FPE_HIP(hipStreamWaitEvent(stream, found->ready, 0));
    }
    return FPE_OK;
}

int prepare_call(fpe_engine* h, const fpe_params* params, float maxRadius, CallPlan& cp, hipStream_t stream, bool wantBits) {
    if (!h || !params) return fail(FPE_E_INVALID_ARG, "null handle or params");
    int rc = fpe::validate_params(*params);
    if (rc != FPE_OK) return fail(rc, "non-finite or negative parameter");
    fpe::Tuning tuning;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        if (!cp.snap) cp.snap = h->map;  // (a snapshot set by the caller stays: prepare_export_layers runs its families on one)
        maxRadius = std::max(maxRadius, std::max(params->searchRadius, h->maxLegSearchRadius));
        tuning = h->tuning;
    }
    if (!cp.snap) return fail(FPE_E_NO_MAP, "no map uploaded");
    MapSnapshot& snap = *cp.snap;
    fpe::PlanConsts& pc = cp.pc;
    fpe::derive_constants(*params, snap.g, maxRadius, tuning, pc);
    if (fpe::spiral_rings(maxRadius, snap.g.res) > h->maxRing)
        return fail(FPE_E_UNSUPPORTED, "search radius needs more spiral rings than the rank table holds");
    pc.defNRings = fpe::spiral_rings(params->searchRadius, snap.g.res);
    pc.defNCand = h->ringStart[static_cast<size_t>(std::min(pc.defNRings, h->maxRing)) + 1];
    cp.planLds = fpe::plan_lds_bytes(pc);
    cp.searchLds = fpe::search_lds_bytes(pc);
    if (cp.planLds > kMaxLdsBytes || cp.searchLds > kMaxLdsBytes)
        return fail(FPE_E_UNSUPPORTED, "search/foot radius too large for the 160 KiB LDS tile");
    FPE_HIP(hipSetDevice(h->device));
    FPE_HIP(snap.wait_ready(stream));
    cp.useBits = wantBits && fpe::bits_supported(pc, snap.g);
    if (cp.useBits) return acquire_mask(snap, pc.thrDefault, pc.thrCandidate, stream, cp);
    return FPE_OK;
}

fpe::DevMap dev_map(const MapSnapshot& s) { return fpe::DevMap{s.g, s.d_trav, s.d_elev}; }

// The region of a dense call: the caller's (row0, col0, n_rows, n_cols), or the whole map for a null `roi`.
int resolve_roi(const int32_t roi[4], const fpe::MapGeom& g, fpe::FootmapRoi& r) {
    if (!roi) {
        r = fpe::FootmapRoi{0, 0, g.rows, g.cols};
        return FPE_OK;
    }
    if (roi[0] < 0 || roi[1] < 0 || roi[2] <= 0 || roi[3] <= 0 || static_cast<int64_t>(roi[0]) + roi[2] > g.rows ||
        static_cast<int64_t>(roi[1]) + roi[3] > g.cols)
        return fail(FPE_E_INVALID_ARG, "region outside the map or empty");
    r = fpe::FootmapRoi{roi[0], roi[1], roi[2], roi[3]};
    return FPE_OK;
}

// fpe_foothold_map*: the snapshot current at entry, the disc constants, the region; `stream` ordered after the snapshot's
// upload and (bit-plane path) its planes' build.  prepare_call's search-radius and plan-LDS bounds do not apply here.
int prepare_foothold_map(fpe_engine* h, const fpe_params* params, const int32_t roi[4], bool anyOut, CallPlan& cp,
                         fpe::FootmapRoi& r, hipStream_t stream) {
    if (!h || !params) return fail(FPE_E_INVALID_ARG, "null handle or params");
    if (!anyOut) return fail(FPE_E_INVALID_ARG, "no output requested");
    int rc = fpe::validate_params(*params);
    if (rc != FPE_OK) return fail(rc, "non-finite or negative parameter");
    fpe::Tuning tuning;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        if (!cp.snap) cp.snap = h->map;  // (as prepare_call)
        tuning = h->tuning;
    }
    if (!cp.snap) return fail(FPE_E_NO_MAP, "no map uploaded");
    MapSnapshot& snap = *cp.snap;
    rc = resolve_roi(roi, snap.g, r);
    if (rc != FPE_OK) return rc;
    fpe::PlanConsts& pc = cp.pc;
    fpe::derive_constants(*params, snap.g, params->searchRadius, tuning, pc);
    if (fpe::foothold_map_supported(pc, snap.g) != FPE_OK)
        return fail(FPE_E_UNSUPPORTED, "foot radius over 32 cells: the literal disc walk is bounded there");
    FPE_HIP(hipSetDevice(h->device));
    FPE_HIP(snap.wait_ready(stream));
    if (pc.footRobust && pc.nHW > 0) return acquire_mask(snap, pc.thrDefault, pc.thrCandidate, stream, cp);
    return FPE_OK;
}

// The snap map's translation-invariance proof (fpe_footsnap.hpp): with p = getPosition(i, j) and a candidate (i + di, j + dj),
// the kernels' f64 comparisons see -di * res, -dj * res and r = double(R) up to a few ulps of the map's coordinates.  Where
// every compared quantity is farther than E from its threshold, the outcome is the same for every cell of the map:
//   rectangle (PNPOLY of getSearchPolygon): inside iff |di| res < r and |dj| res < r / 2  ->  |di| <= rectA, |dj| <= rectB;
//   ring filter of rings nRings - 1, nRings (isInside): (di^2 + dj^2) res^2 <= r^2        ->  di^2 + dj^2 <= ringT.
// Returns false when some threshold lies within E of a lattice value (e.g. r / res whole with r and res exact binary fractions).
bool snap_prove(const fpe::MapGeom& g, fpe::SnapConsts& sc) {
    const double res = g.res, r = static_cast<double>(sc.Rf);
    const double ext = std::max(std::max(std::fabs(g.baseX), std::fabs(fpe::cell_pos(g.baseX, res, g.rows - 1))),
                                std::max(std::fabs(g.baseY), std::fabs(fpe::cell_pos(g.baseY, res, g.cols - 1)))) + r + res;
    const double E = 64.0 * DBL_EPSILON * (1.0 + ext);
    auto half = [&](double hr, int32_t& A) {
        int a = static_cast<int>(std::floor(hr / res));
        while (a >= 0 && a * res >= hr) --a;
        while ((a + 1) * res < hr) ++a;
        A = a;
        return std::fabs(a * res - hr) > E && std::fabs((a + 1) * res - hr) > E;
    };
    bool ok = half(r, sc.rectA);
    ok = half(0.5 * r, sc.rectB) && ok;
    const double E2 = 2.0 * (r + 2.0 * res) * E + E * E;
    sc.ringT = -1;
    for (int n = 0; n <= 2 * (sc.nRings + 1) * (sc.nRings + 1); ++n) {
        const double d2 = static_cast<double>(n) * res * res;
        if (std::fabs(d2 - r * r) <= E2) ok = false;
        if (d2 <= r * r) sc.ringT = n;
    }
    return ok;
}

// fpe_foothold_snap*: prepare_call for the search radius (the tile, the ring bound and the LDS bound of fpe_search_legs: what it
// would report as source 3 is FPE_E_UNSUPPORTED here), the region, the snap constants and the path; `stream` ordered after the
// snapshot's upload and (bit path) its planes' build.
int prepare_foothold_snap(fpe_engine* h, const fpe_params* params, const int32_t roi[4], float searchRadius, int32_t polygonKind,
                          bool anyOut, bool wantZ, CallPlan& cp, fpe::FootmapRoi& r, fpe::SnapConsts& sc, bool& bitPath,
                          hipStream_t stream) {
    if (!h || !params) return fail(FPE_E_INVALID_ARG, "null handle or params");
    if (!anyOut) return fail(FPE_E_INVALID_ARG, "no output requested");
    if (polygonKind != 0 && polygonKind != 1) return fail(FPE_E_INVALID_ARG, "polygon_kind must be 0 (rectangle) or 1 (hexagon)");
    if (!std::isfinite(searchRadius)) return fail(FPE_E_INVALID_ARG, "bad search radius");
    const float R = searchRadius > 0.0f ? searchRadius : params->searchRadius;
    int rc = prepare_call(h, params, R, cp, stream, false);
    if (rc != FPE_OK) return rc;
    const fpe::MapGeom& g = cp.snap->g;
    rc = resolve_roi(roi, g, r);
    if (rc != FPE_OK) return rc;
    const fpe::PlanConsts& pc = cp.pc;
    if (wantZ && fpe::foothold_map_supported(pc, g) != FPE_OK)
        return fail(FPE_E_UNSUPPORTED, "foot radius over 32 cells: the literal disc walk is bounded there");
    sc.Rf = R;
    sc.polyKind = polygonKind;
    sc.nRings = fpe::spiral_rings(R, g.res);
    sc.nCand = h->ringStart[static_cast<size_t>(std::min(sc.nRings, h->maxRing)) + 1];
    const bool proved = snap_prove(g, sc);
    bitPath = fpe::foothold_snap_bits_ok(pc, sc, true, proved);
    if (bitPath) return acquire_mask(*cp.snap, pc.thrDefault, pc.thrCandidate, stream, cp);
    return FPE_OK;
}

// Queue the products of a prepared snap call on `stream` (the literal path's scratch is stream-ordered).
hipError_t run_foothold_snap(fpe_engine* h, const CallPlan& cp, const fpe::FootmapRoi& r, const fpe::SnapConsts& sc, bool bitPath,
                             int8_t* d_offset, uint8_t* d_source, float* d_z, hipStream_t stream) {
    if (bitPath) return fpe::launch_foothold_snap_bits(dev_map(*cp.snap), cp.bits, cp.pc, sc, h->lut(), r, d_offset, d_source, d_z, stream);
    void* scratch = nullptr;
    hipError_t e = hipMallocAsync(&scratch, fpe::foothold_snap_literal_scratch_bytes(), stream);
    if (e != hipSuccess) return e;
    e = fpe::launch_foothold_snap_literal(dev_map(*cp.snap), cp.pc, sc, h->lut(), r, scratch, d_offset, d_source, d_z, stream);
    const hipError_t f = hipFreeAsync(scratch, stream);
    return e != hipSuccess ? e : f;
}

// fpe_centroid_map*: prepare_call (the plan constants of the disc functions), the region and the dense constants; `stream`
// ordered after the snapshot's upload.  A rectangle over the dense kernels' reach is FPE_E_UNSUPPORTED.
int prepare_centroid_map(fpe_engine* h, const fpe_params* params, const int32_t roi[4], float searchRadius, bool anyOut, CallPlan& cp,
                         fpe::FootmapRoi& r, fpe::CmapConsts& cc, hipStream_t stream) {
    if (!h || !params) return fail(FPE_E_INVALID_ARG, "null handle or params");
    if (!anyOut) return fail(FPE_E_INVALID_ARG, "no output requested");
    if (!std::isfinite(searchRadius)) return fail(FPE_E_INVALID_ARG, "bad search radius");
    int rc = prepare_call(h, params, 0.0f, cp, stream, false);
    if (rc != FPE_OK) return rc;
    const fpe::MapGeom& g = cp.snap->g;
    rc = resolve_roi(roi, g, r);
    if (rc != FPE_OK) return rc;
    const float R = searchRadius > 0.0f ? searchRadius : params->searchRadius;
    if (!fpe::centroid_map_consts(g, r, R, cc))
        return fail(FPE_E_UNSUPPORTED, "search radius over the dense centroid map's reach (ceil(R / res) + 2 > 100 cells)");
    return FPE_OK;
}

// Queue the products of a prepared dense centroid call on `stream` (its scratch is stream-ordered)
hipError_t run_centroid_map(const CallPlan& cp, const fpe::FootmapRoi& r, const fpe::CmapConsts& cc, uint8_t* d_code, int8_t* d_offset,
                            float* d_z, hipStream_t stream) {
    void* scratch = nullptr;
    hipError_t e = hipMallocAsync(&scratch, fpe::centroid_map_scratch_bytes(r, cc), stream);
    if (e != hipSuccess) return e;
    e = fpe::launch_centroid_map(dev_map(*cp.snap), cp.pc, cc, r, scratch, d_code, d_offset, d_z, stream);
    const hipError_t f = hipFreeAsync(scratch, stream);
    return e != hipSuccess ? e : f;
}

// Every *_device entry point calls this after a successful prepare and BEFORE its launch.  The launch is asynchronous: the host never
// waits for it, so the snapshot's layers and the bit planes the call launches with may be recycled only behind a device
// synchronisation (BufferPool; the planes directly, not by way of the snapshot's mark — a set evicted by a fifth threshold pair no
// longer hears of that one).  Before the launch, so that no way out of the entry point leaves work queued on buffers that count as
// clean; a launch that then fails leaves them dirty too: one synchronisation on a 10-20 Hz path, never on a plan.
void mark_async_launch(const CallPlan& cp) {
    cp.snap->note_async_use();
    if (cp.mask) cp.mask->asyncUsed.store(true, std::memory_order_release);
}

// What a host-buffer call holds while it runs.  The member order is the point: the lease goes first, so on an early exit it waits
// for the stream BEFORE the snapshot / bit planes are released (every host-buffer entry point, plan_host included, holds both here).
struct HostCall {
    CallPlan cp;
    CtxLease lease;
    CallCtx& cx;
    explicit HostCall(fpe_engine* h) : lease(h->ctxPool), cx(*lease.ctx) {}
};

// One product of a dense host-form call: the caller's array and its length in bytes (null or 0: not requested).
struct HostProduct {
    void* dst;
    size_t len;
};

// The host form of a dense call behind its prepare: the requested products side by side in the context's device arena (256-byte
// steps), `launch(d, stream)` queues the kernels (d[k]: where product k goes, null when not requested), one DMA transfer per product
// — straight into a pinned destination, into the pinned arena for any other — one synchronisation, the staged products copied out.
template <int N, class Launch>
int stage_products(CallCtx& cx, const HostProduct (&prod)[N], Launch launch) {
    size_t len[N], off[N], end = 0;
    bool pinned[N];
    for (int k = 0; k < N; ++k) {
        len[k] = prod[k].dst ? prod[k].len : 0;
        pinned[k] = len[k] && is_pinned_host(prod[k].dst);
        off[k] = end;
        end = align256(end + len[k]);
    }
    FPE_HIP(cx.reserve(end));
    unsigned char* d[N];
    for (int k = 0; k < N; ++k) d[k] = len[k] ? cx.dev + off[k] : nullptr;
    cx.inFlight = true;
    FPE_HIP(launch(d, cx.stream));
    for (int k = 0; k < N; ++k)
        if (len[k]) FPE_HIP(hipMemcpyAsync(pinned[k] ? prod[k].dst : cx.pinned + off[k], d[k], len[k], hipMemcpyDeviceToHost, cx.stream));
    FPE_HIP(hipStreamSynchronize(cx.stream));
    cx.inFlight = false;
    for (int k = 0; k < N; ++k)
        if (len[k] && !pinned[k]) std::memcpy(prod[k].dst, cx.pinned + off[k], len[k]);
    return FPE_OK;
}

// fpe_export_layers*: what a layer id reads — its dense family, that family's canonical product and how layers_export_kernel
// reads it (fpe_launch.hpp).  One line per FPE_LAYER_* id of include/fpe.h, in id order.
enum ExportFamily { kFamFootmap, kFamSnap, kFamCentroid, kExportFamilies };
enum ExportProduct { kXpFlags, kXpHeight, kXpSnapOffset, kXpSnapSource, kXpSnapZ, kXpCenCode, kXpCenOffset, kXpCenZ, kExportProducts };
struct ExportLayerDef {
    int family, product, kind;
};
constexpr ExportLayerDef kExportLayers[FPE_LAYER_COUNT] = {
    {kFamFootmap, kXpFlags, fpe::kLayerSrcU8},             // FPE_LAYER_FOOTHOLD_FLAGS
    {kFamFootmap, kXpHeight, fpe::kLayerSrcF32},           // FPE_LAYER_FOOTHOLD_HEIGHT
    {kFamSnap, kXpSnapOffset, fpe::kLayerSrcI8Pair0},      // FPE_LAYER_SNAP_DI
    {kFamSnap, kXpSnapOffset, fpe::kLayerSrcI8Pair1},      // FPE_LAYER_SNAP_DJ
    {kFamSnap, kXpSnapSource, fpe::kLayerSrcU8},           // FPE_LAYER_SNAP_SOURCE
    {kFamSnap, kXpSnapZ, fpe::kLayerSrcF32},               // FPE_LAYER_SNAP_Z
    {kFamCentroid, kXpCenCode, fpe::kLayerSrcU8},          // FPE_LAYER_CENTROID_CODE
    {kFamCentroid, kXpCenOffset, fpe::kLayerSrcI8Pair0},   // FPE_LAYER_CENTROID_DI
    {kFamCentroid, kXpCenOffset, fpe::kLayerSrcI8Pair1},   // FPE_LAYER_CENTROID_DJ
    {kFamCentroid, kXpCenZ, fpe::kLayerSrcF32},            // FPE_LAYER_CENTROID_Z
};
constexpr size_t kExportProductBytes[kExportProducts] = {1, 4, 2, 1, 4, 1, 2, 4};  // per cell of the region

// A prepared export call.  One snapshot; a CallPlan per family, because the families derive different plan constants from the
// same parameters (the snap map sizes its tile for its own radius, the centroid map for the engine's leg bound, the foothold map
// for params->searchRadius) and every product has to be exactly its own dense call's.  The foothold map and the snap map ask for the
// same threshold pair: the second acquire_mask finds the first one's planes.
struct ExportPlan {
    CallPlan cp[kExportFamilies];
    bool prepared[kExportFamilies] = {};  // the family is requested and its prepare succeeded
    bool want[kExportProducts] = {};
    fpe::FootmapRoi r{};
    fpe::SnapConsts sc{};
    bool bitPath = false;
    fpe::CmapConsts cc{};
    fpe::LayersArgs args{};  // everything but the slots' pointers
};

// Every check of an export call, then the prepares of the families requested on ONE snapshot; `stream` ordered as they order it.
// The centroid map (no bit planes) goes first and the foothold map last, so that as few refusals as possible come behind a queued
// build of the planes; xp.prepared tells the device form which plans a refusal leaves to mark.
int prepare_export_layers(fpe_engine* h, const fpe_params* params, const int32_t roi[4], const fpe_layer_layout* layout,
                          const fpe_layer_request* req, ExportPlan& xp, hipStream_t stream) {
    if (!h || !params || !req) return fail(FPE_E_INVALID_ARG, "null handle, params or request");
    if (req->n_layers < 1 || req->n_layers > FPE_LAYER_COUNT) return fail(FPE_E_INVALID_ARG, "n_layers must be 1..FPE_LAYER_COUNT");
    bool need[kExportFamilies] = {};
    uint32_t seen = 0;
    for (int k = 0; k < req->n_layers; ++k) {
        const int32_t id = req->layer[k];
        if (id < 0 || id >= FPE_LAYER_COUNT) return fail(FPE_E_INVALID_ARG, "unknown layer id");
        if ((seen >> id) & 1u) return fail(FPE_E_INVALID_ARG, "layer requested twice");
        seen |= 1u << id;
        if (!req->dst[k]) return fail(FPE_E_INVALID_ARG, "null layer destination");
        need[kExportLayers[id].family] = true;
        xp.want[kExportLayers[id].product] = true;
    }
    const int32_t si = layout ? layout->start_index[0] : 0, sj = layout ? layout->start_index[1] : 0;
    const int32_t order = layout ? layout->storage_order : 1;
    if (order != 0 && order != 1) return fail(FPE_E_INVALID_ARG, "storage_order must be 0 (column-major) or 1 (row-major)");
    std::shared_ptr<MapSnapshot> snap;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        snap = h->map;
    }
    if (!snap) return fail(FPE_E_NO_MAP, "no map uploaded");
    const fpe::MapGeom& g = snap->g;
    if (si < 0 || si >= g.rows || sj < 0 || sj >= g.cols) return fail(FPE_E_INVALID_ARG, "start index outside the map");
    int rc = resolve_roi(roi, g, xp.r);
    if (rc != FPE_OK) return rc;
    if (need[kFamCentroid]) {
        xp.cp[kFamCentroid].snap = snap;
        rc = prepare_centroid_map(h, params, roi, req->centroid_search_radius, true, xp.cp[kFamCentroid], xp.r, xp.cc, stream);
        if (rc != FPE_OK) return rc;
        xp.prepared[kFamCentroid] = true;
    }
    if (need[kFamSnap]) {
        xp.cp[kFamSnap].snap = snap;
        rc = prepare_foothold_snap(h, params, roi, req->snap_search_radius, req->snap_polygon_kind, true, xp.want[kXpSnapZ], xp.cp[kFamSnap],
                                   xp.r, xp.sc, xp.bitPath, stream);
        if (rc != FPE_OK) return rc;
        xp.prepared[kFamSnap] = true;
    }
    if (need[kFamFootmap]) {
        xp.cp[kFamFootmap].snap = snap;
        rc = prepare_foothold_map(h, params, roi, true, xp.cp[kFamFootmap], xp.r, stream);
        if (rc != FPE_OK) return rc;
        xp.prepared[kFamFootmap] = true;
    }
    fpe::LayersArgs& a = xp.args;
    a.rows = g.rows;
    a.cols = g.cols;
    a.si = si;
    a.sj = sj;
    a.dstRowMajor = order;
    a.nLayers = req->n_layers;
    a.roi = xp.r;
    return FPE_OK;
}

// Queue a prepared export call on `stream`: the canonical products the layers need in one stream-ordered block, the dense
// families' own launches into it, then ONE launch of layers_export_kernel into d_dst[k] (device; layer req.layer[k]).
hipError_t run_export_layers(fpe_engine* h, const ExportPlan& xp, const fpe_layer_request& req, float* const* d_dst, hipStream_t stream) {
    const size_t n = static_cast<size_t>(xp.r.nr) * xp.r.nc;
    size_t off[kExportProducts], end = 0;
    for (int p = 0; p < kExportProducts; ++p) {
        off[p] = end;
        if (xp.want[p]) end = align256(end + n * kExportProductBytes[p]);
    }
    void* block = nullptr;
    hipError_t e = hipMallocAsync(&block, end, stream);
    if (e != hipSuccess) return e;
    unsigned char* base = static_cast<unsigned char*>(block);
    auto at = [&](int p) { return xp.want[p] ? base + off[p] : nullptr; };
    if (xp.prepared[kFamFootmap]) {
        const CallPlan& cp = xp.cp[kFamFootmap];
        e = fpe::launch_foothold_map(dev_map(*cp.snap), cp.bits, cp.pc, xp.r, at(kXpFlags), reinterpret_cast<float*>(at(kXpHeight)), stream);
    }
    if (e == hipSuccess && xp.prepared[kFamSnap])
        e = run_foothold_snap(h, xp.cp[kFamSnap], xp.r, xp.sc, xp.bitPath, reinterpret_cast<int8_t*>(at(kXpSnapOffset)), at(kXpSnapSource),
                              reinterpret_cast<float*>(at(kXpSnapZ)), stream);
    if (e == hipSuccess && xp.prepared[kFamCentroid])
        e = run_centroid_map(xp.cp[kFamCentroid], xp.r, xp.cc, at(kXpCenCode), reinterpret_cast<int8_t*>(at(kXpCenOffset)),
                             reinterpret_cast<float*>(at(kXpCenZ)), stream);
    if (e == hipSuccess) {
        fpe::LayersArgs a = xp.args;
        for (int k = 0; k < a.nLayers; ++k) {
            const ExportLayerDef& d = kExportLayers[req.layer[k]];
            a.slot[k] = fpe::LayerSlot{at(d.product), d_dst[k], d.kind, 0};
        }
        e = fpe::launch_layers_export(a, stream);
    }
    const hipError_t f = hipFreeAsync(block, stream);
    return e != hipSuccess ? e : f;
}

// The host form of an open-loop query call behind its per-query checks: n queries up, `launch(cp, d_queries, d_out, stream)`,
// n records back, both through the context's arenas.  check (a function pointer, which may be null, or any callable): a refusal that
// needs the call's snapshot, ahead of any copy.
template <class Query, class Record, class Launch, class Check = int (*)(const CallPlan&)>
int query_round_trip(fpe_engine* h, const fpe_params* params, float maxRadius, const Query* queries, int32_t n, Record* out, Launch launch,
                     Check check = nullptr) {
    if (!h) return fail(FPE_E_INVALID_ARG, "null handle or params");
    const size_t nQ = static_cast<size_t>(n) * sizeof(Query), nO = static_cast<size_t>(n) * sizeof(Record);
    const size_t szQ = align256(nQ);
    HostCall hc(h);
    CallCtx& cx = hc.cx;
    FPE_HIP(hipSetDevice(h->device));
    FPE_HIP(cx.reserve(szQ + align256(nO)));
    cx.inFlight = true;
    int rc = prepare_call(h, params, maxRadius, hc.cp, cx.stream, false);
    if constexpr (std::is_pointer_v<Check>) {
        if (rc == FPE_OK && check) rc = check(hc.cp);
    } else {
        if (rc == FPE_OK) rc = check(hc.cp);
    }
    if (rc != FPE_OK) return rc;
    std::memcpy(cx.pinned, queries, nQ);
    FPE_HIP(hipMemcpyAsync(cx.dev, cx.pinned, nQ, hipMemcpyHostToDevice, cx.stream));
    FPE_HIP(launch(hc.cp, reinterpret_cast<const Query*>(cx.dev), reinterpret_cast<Record*>(cx.dev + szQ), cx.stream));
    FPE_HIP(hipMemcpyAsync(cx.pinned + szQ, cx.dev + szQ, nO, hipMemcpyDeviceToHost, cx.stream));
    FPE_HIP(hipStreamSynchronize(cx.stream));
    cx.inFlight = false;
    std::memcpy(out, cx.pinned + szQ, nO);
    return FPE_OK;
}

// The products of a plan call and the slots() views of fpe_plan_out / fpe_opt_out: the product table of fpe_launch.hpp
using fpe::kCycleOk;
using fpe::kOptProducts;
using fpe::kPlanProducts;
using fpe::kProducts;
using fpe::product_bytes;
using fpe::slots;

// selected_packed holds biased 14-bit grid indices: wherever the product is asked for, a larger map is refused.
int check_packed_fits(const CallPlan& cp, bool wanted) {
    if (wanted && (cp.snap->g.rows > FPE_PACKED_MAX_CELLS || cp.snap->g.cols > FPE_PACKED_MAX_CELLS))
        return fail(FPE_E_UNSUPPORTED, "selected_packed holds biased 14-bit grid indices: the map has more than 15871 rows or columns");
    return FPE_OK;
}

// One result of a host-form plan / ranking call: `len` bytes at offset `off` of the call's arenas (device and pinned: the same
// offsets in both), wanted at `dst`.  A list holds them in arena order.
struct Seg {
    size_t off, len;
    void* dst;
};
constexpr int kMaxSegs = kPlanProducts + 5 + 6;  // the longest list: a checked beam's products, beam outputs and check outputs
static_assert(kProducts + 1 <= kMaxSegs, "SegList holds a resume call's products and its state");
struct SegList {
    Seg s[kMaxSegs];  // (a ranking call: its eight products and four outputs of its own, checked: five more; a beam call: five, checked: six more; a resume call: the state as well)
    int n = 0;
    void add(size_t off, size_t len, void* dst) {
        if (dst && len) s[n++] = Seg{off, len, dst};
    }
};
// Every result is in the pinned arena (the kernels of a zero-copy call wrote it there themselves): out to the caller.
void copy_from_pinned(const SegList& segs, const unsigned char* pinned) {
    for (int k = 0; k < segs.n; ++k) std::memcpy(segs.s[k].dst, pinned + segs.s[k].off, segs.s[k].len);
}

// The cursor of a ranking / beam call's layout over its two blocks, in offsets: the scratch (256-byte steps) and — the host form —
// the output block, whose transfers to the caller it lists as it goes (outs: offsets in the call's arenas, the block at outOff0).
// A layout runs twice: without bases for the sizes (null comes back, nothing is added to a null pointer), then on the bases.
struct ArenaCursor {
    unsigned char* base = nullptr;     // the scratch
    unsigned char* outBase = nullptr;  // the output block, as the kernels see it
    size_t outOff0 = 0;
    size_t scratchBytes = 0, outBytes = 0;
    SegList outs;
    void* take(size_t bytes) {
        const size_t off = scratchBytes;
        scratchBytes += align256(bytes);
        return base ? base + off : nullptr;
    }
    template <class T>
    T* take_n(size_t n) {
        return static_cast<T*>(take(n * sizeof(T)));
    }
    void* out(void* callerDst, size_t bytes) {
        const size_t off = outBytes;
        outBytes += align256(bytes);
        outs.add(outOff0 + off, bytes, callerDst);
        return outBase ? outBase + off : nullptr;
    }
};

// The tail of a device-form call: `run(scratch)` queues its launches on `bytes` of stream-ordered scratch; its error goes ahead of
// the free's.
template <class Run>
int with_stream_scratch(size_t bytes, hipStream_t stream, Run run) {
    void* scratch = nullptr;
    FPE_HIP(hipMallocAsync(&scratch, bytes, stream));
    const int rc = run(static_cast<unsigned char*>(scratch));
    const hipError_t f = hipFreeAsync(scratch, stream);
    if (rc != FPE_OK) return rc;
    FPE_HIP(f);
    return FPE_OK;
}

// The results of a host-form call from the device arena `dev` to the caller, behind the kernels queued on cx.stream; `pinned`: the
// pinned arena (the staging area).  Ends synchronised.  The list comes by value: a segment that has left directly loses its `dst`.
// Only what the caller asked for crosses PCIe.  A product whose destination is pinned / registered host memory
// (fpe_host_alloc) is written by DMA directly; the others go through the pinned arena in chunks, and the copy of a
// chunk into the caller's array runs on the copy pool while the next chunks are still in flight.
// Pinned destinations that lie behind one another exactly as the products do in the device arena (no padding in between:
// FootholdPlanner.plan_outputs(pinned=True) carves them out of ONE fpe_host_alloc block in this order) leave in ONE copy:
// a DMA transfer has a fixed cost of some ten microseconds, and seven of them in a row are a third of a 4 096-pose call.
int copy_out(fpe_engine* h, CallCtx& cx, SegList list, const unsigned char* dev, unsigned char* pinned) {
    Seg* const segs = list.s;
    const int nSeg = list.n;
    size_t staged = 0;
    bool pinnedSeg[kMaxSegs];
    for (int k = 0; k < nSeg; ++k) pinnedSeg[k] = is_pinned_host(segs[k].dst);
    for (int k = 0; k < nSeg; ++k) {
        if (!pinnedSeg[k]) {
            staged += segs[k].len;
            continue;
        }
        size_t len = segs[k].len;
        int last = k;
        while (last + 1 < nSeg && pinnedSeg[last + 1] && segs[last + 1].off == segs[last].off + segs[last].len &&
               static_cast<unsigned char*>(segs[last + 1].dst) == static_cast<unsigned char*>(segs[last].dst) + segs[last].len) {
            ++last;
            len += segs[last].len;
        }
        FPE_HIP(hipMemcpyAsync(segs[k].dst, dev + segs[k].off, len, hipMemcpyDeviceToHost, cx.stream));
        for (int q = k; q <= last; ++q) segs[q].dst = nullptr;
        k = last;
    }
    // A DMA transfer has a fixed cost of some ten microseconds: few, large pieces (a quarter of what is staged, at least
    // 1 MB), and the copy of a piece into the caller's array split over the pool's threads so that the last piece's copy — the
    // only one that is not hidden behind a later transfer — is short.
    constexpr size_t kTargetChunks = 4;
    const size_t chunk = std::max<size_t>(1u << 20, (staged / kTargetChunks + 4095) & ~static_cast<size_t>(4095));
    // DMA pieces are cut from RUNS of staged products that are neighbours in the arena (alignment padding rides along: both
    // arenas are the engine's own), not from single products: four transfers for seven products, not nine.
    struct Piece {
        size_t off, len;
    };
    std::vector<Piece> pieces;
    for (int k = 0; k < nSeg; ++k) {
        if (!segs[k].dst) continue;
        int last = k;
        while (last + 1 < nSeg && segs[last + 1].dst && segs[last + 1].off == align256(segs[last].off + segs[last].len)) ++last;
        const size_t end = segs[last].off + segs[last].len;
        for (size_t c = segs[k].off; c < end; c += chunk) pieces.push_back(Piece{c, std::min(chunk, end - c)});
        k = last;
    }
    for (size_t k = 0; k < pieces.size(); ++k) {
        hipEvent_t ev;
        FPE_HIP(cx.event(k, &ev));
        FPE_HIP(hipMemcpyAsync(pinned + pieces[k].off, dev + pieces[k].off, pieces[k].len, hipMemcpyDeviceToHost, cx.stream));
        FPE_HIP(hipEventRecord(ev, cx.stream));
    }
    CopyPool::Batch batch;
    hipError_t evErr = hipSuccess;
    for (size_t k = 0; k < pieces.size(); ++k) {
        const hipError_t e = hipEventSynchronize(cx.events[k]);
        if (e != hipSuccess) {
            evErr = e;
            break;
        }
        // what the piece holds of each staged product, into the caller's array
        const size_t p0 = pieces[k].off, p1 = p0 + pieces[k].len;
        for (int q = 0; q < nSeg; ++q) {
            if (!segs[q].dst) continue;
            const size_t a0 = std::max(p0, segs[q].off), a1 = std::min(p1, segs[q].off + segs[q].len);
            if (a0 >= a1) continue;
            unsigned char* dst = static_cast<unsigned char*>(segs[q].dst) + (a0 - segs[q].off);
            const size_t len = a1 - a0;
            if (len >= (256u << 10)) {
                const size_t parts = std::min<size_t>(h->copyPool.width(), (len + (256u << 10) - 1) / (256u << 10));
                const size_t step = ((len + parts - 1) / parts + 63) & ~static_cast<size_t>(63);
                for (size_t c = 0; c < len; c += step) h->copyPool.submit(batch, dst + c, pinned + a0 + c, std::min(step, len - c));
            } else {
                std::memcpy(dst, pinned + a0, len);
            }
        }
    }
    CopyPool::wait(batch);
    if (evErr != hipSuccess) return fail_hip(evErr, "result copy");  // (the lease waits for the stream)
    FPE_HIP(hipStreamSynchronize(cx.stream));  // the direct (pinned-destination) copies
    cx.inFlight = false;
    return FPE_OK;
}

int check_desc(const fpe_map_desc* d) {
    if (!d) return fail(FPE_E_INVALID_ARG, "null map descriptor");
    const char* why = "";
    const int rc = fpe::check_map_geometry(d->rows, d->cols, d->resolution, &why);
    if (rc != FPE_OK) return fail(rc, why);
    if (!std::isfinite(d->position[0]) || !std::isfinite(d->position[1])) return fail(FPE_E_INVALID_ARG, "bad position");
    if (d->start_index[0] < 0 || d->start_index[0] >= d->rows || d->start_index[1] < 0 || d->start_index[1] >= d->cols)
        return fail(FPE_E_INVALID_ARG, "start index out of range");
    if (d->storage_order != 0 && d->storage_order != 1) return fail(FPE_E_INVALID_ARG, "bad storage order");
    return FPE_OK;
}

// The step_height buffer of one traversability-only chain on `stream` (fpe_engine::filterSlots), with the GPU-side wait it may need
// queued.  The caller holds h->filterMu from here until its chain is QUEUED and filter_slot_done has recorded the slot's event.
int filter_slot_take(fpe_engine* h, size_t n, hipStream_t stream, fpe_engine::FilterSlot*& slot) {
    slot = nullptr;
    bool wait = false;
    for (auto& fs : h->filterSlots)  // (1) this stream's own buffer
        if (fs.buf && fs.cap >= n && fs.cap <= 4 * n + 4096 && fs.last == stream && (!slot || fs.use > slot->use)) slot = &fs;
    // (the wait on the slot's event is queued in this case too: on the same in-order queue it is free, and a caller who destroyed
    // the stream with work pending and got the same handle value back for a new one is ordered behind the old chain — ADVICE r5)
    if (slot) wait = true;
    if (!slot)
        for (auto& fs : h->filterSlots)  // (2) an idle buffer
            if (fs.buf && fs.cap >= n && fs.cap <= 4 * n + 4096 && hipEventQuery(fs.done) == hipSuccess) {
                slot = &fs;
                break;
            }
    (void)hipGetLastError();  // hipErrorNotReady of the queries above is not an error
    if (!slot) {
        for (auto& fs : h->filterSlots)  // (3) a free slot, else (4) the least recently used one
            if (!fs.buf) {
                slot = &fs;
                break;
            }
        if (!slot) {
            slot = &h->filterSlots[0];
            for (auto& fs : h->filterSlots)
                if (fs.use < slot->use) slot = &fs;
            wait = true;
        }
        if (slot->buf && slot->cap < n) {  // too small (also reached by (4)): back to the pool, dirty — its last chain may still run
            h->pool->give(slot->cap, slot->buf, true);
            slot->buf = nullptr;
            wait = false;
        }
        if (!slot->buf) FPE_HIP(alloc_units(*h->pool, n, &slot->buf, &slot->cap, true));  // cleanOnly: never a device synchronisation
        if (!slot->done) FPE_HIP(hipEventCreateWithFlags(&slot->done, hipEventDisableTiming));
    }
    if (wait) FPE_HIP(hipStreamWaitEvent(stream, slot->done, 0));
    return FPE_OK;
}
// Behind the chain that used `slot` — or behind whatever part of it was queued when a later step failed: the event its next user
// waits for is recorded on every way out (a slot left without one would let that user run beside this chain's kernels).
hipError_t filter_slot_done(fpe_engine* h, fpe_engine::FilterSlot* slot, hipStream_t stream) {
    const hipError_t e = hipEventRecord(slot->done, stream);
    slot->last = stream;
    slot->use = ++h->filterClock;
    return e;
}

// ---- what a full upload (upload_common) and an incremental update (update_common) share ----------------------------------------
// A snapshot of this geometry with both layers from the pool, not yet filled.
int new_snapshot(fpe_engine* h, int rows, int cols, double res, double posX, double posY, std::shared_ptr<MapSnapshot>& out) {
    auto snap = std::make_shared<MapSnapshot>();
    snap->g = fpe::make_geom(rows, cols, res, posX, posY);
    snap->n = static_cast<size_t>(rows) * cols;
    snap->pool = h->pool;
    FPE_HIP(alloc_units(*h->pool, snap->n, &snap->d_trav, &snap->capTrav));
    FPE_HIP(alloc_units(*h->pool, snap->n, &snap->d_elev, &snap->capElev));
    out = std::move(snap);
    return FPE_OK;
}
// Threshold pairs `cur` (the snapshot being replaced; may be null) was planned with: the new snapshot gets their planes at once.
std::vector<std::pair<float, float>> carried_pairs(const std::shared_ptr<MapSnapshot>& cur) {
    std::vector<std::pair<float, float>> pairs;
    if (cur) {
        std::lock_guard<std::mutex> lk(cur->mu);
        for (auto& ms : cur->masks) pairs.emplace_back(ms->thrD, ms->thrC);
    }
    return pairs;
}
// The plane buffer of a pair whose planes are written by the kernel that moves the traversability layer.  That kernel writes the
// buffer asynchronously: should any later step fail, the buffer goes back to the pool DIRTY (its next taker synchronises) — a dirty
// return costs a synchronisation, a clean one of a buffer with work queued on it would be a race.  Cleared again by
// folded_ready.
int alloc_folded(MapSnapshot& snap, const std::pair<float, float>& pair, std::shared_ptr<MaskSet>& out) {
    const int rc = alloc_mask(snap, pair.first, pair.second, false, out);
    if (rc != FPE_OK) return rc;
    out->asyncUsed.store(true, std::memory_order_release);
    return FPE_OK;
}
// Behind the kernel that wrote `folded`: its event, and into the snapshot's sets.
int folded_ready(MapSnapshot& snap, const std::shared_ptr<MaskSet>& folded, hipStream_t stream) {
    const int rc = mask_ready(*folded, stream);
    if (rc != FPE_OK) return rc;
    // from here on ~MaskSet waits for `ready` (recorded behind the kernel that wrote the planes) before it gives the buffer back
    folded->asyncUsed.store(false, std::memory_order_release);
    folded->lastUse.store(++snap.useClock);
    snap.masks.push_back(folded);
    return FPE_OK;
}
// `snap`, filled on `stream` with its `ready` recorded, becomes the engine's current snapshot.
int install_snapshot(fpe_engine* h, std::shared_ptr<MapSnapshot>& snap, bool hostForm, hipStream_t stream) {
    // A host-buffer upload is synchronous already (the caller's arrays may be freed on return): it also waits for the planes it
    // has just queued, so the snapshot it installs is COMPLETE and the first service call on the new map waits for nothing
    // (bench.py service_latency_us: first_call_after_a_map was 16 us above steady_map — the plane build and its event on the
    // call's critical path; the map stream is the 10-20 Hz path that can afford it).
    if (hostForm && !snap->masks.empty()) {
        FPE_HIP(hipStreamSynchronize(stream));
        for (auto& ms : snap->masks) ms->readyDone.store(true, std::memory_order_release);
    }
    // (a host form has synchronised behind its copies and kernels: the snapshot is known complete — its first consumer need not ask the event)
    if (hostForm) snap->readyDone.store(true, std::memory_order_release);
    std::shared_ptr<MapSnapshot> old;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        old = std::move(h->map);
        h->map = snap;  // readers holding the old snapshot keep it alive until they finish
    }
    old.reset();  // outside the engine lock: ~MapSnapshot may wait for the old snapshot's last asynchronous readers
    return FPE_OK;
}

int upload_common(fpe_engine* h, const fpe_map_desc* desc, const float* trav, const float* elev, bool srcOnDevice,
                  hipStream_t stream) {
    if (!h || !trav || !elev) return fail(FPE_E_INVALID_ARG, "null argument");
    int rc = check_desc(desc);
    if (rc != FPE_OK) return rc;
    FPE_HIP(hipSetDevice(h->device));
    const size_t n = static_cast<size_t>(desc->rows) * desc->cols;
    std::shared_ptr<MapSnapshot> snap;
    rc = new_snapshot(h, desc->rows, desc->cols, desc->resolution, desc->position[0], desc->position[1], snap);
    if (rc != FPE_OK) return rc;
    const bool canonical = desc->storage_order == 1 && desc->start_index[0] == 0 && desc->start_index[1] == 0;
    const float* src[2] = {trav, elev};
    float* dst[2] = {snap->d_trav, snap->d_elev};
    // staging layer of a host upload in message layout (handed back clean: a host upload waits for its stream layer by layer)
    PooledBuf stagingGuard{h->pool, false};
    float*& staging = stagingGuard.p;
    if (!srcOnDevice && !canonical) FPE_HIP(stagingGuard.take(n));
    // Threshold pairs the CURRENT snapshot was planned with: their bit planes are built here, on the upload's stream — the
    // upload is the 10-20 Hz path that may take a recycled ("dirty") buffer behind a device synchronisation; the first plan on
    // the new map then finds its planes and pays nothing (include/fpe.h: "plans never pay for it").  The FIRST pair's planes
    // ride in the kernel that moves the traversability layer anyway (canonicalise_layer_kernel ballots every destination row it
    // holds; round 5) whenever the layer goes through a kernel — message layout, or a device source (then the kernel replaces
    // the device-to-device copy): no second pass over the layer.  Further pairs (rare) by build_bitmap_kernel.
    std::vector<std::pair<float, float>> pairs;
    {
        std::shared_ptr<MapSnapshot> cur;
        {
            std::lock_guard<std::mutex> lk(h->mu);
            cur = h->map;
        }
        pairs = carried_pairs(cur);
    }
    std::shared_ptr<MaskSet> folded;
    const bool travThroughKernel = !canonical || srcOnDevice;
    if (!pairs.empty() && travThroughKernel && desc->rows < (1 << 24) - 2 && desc->cols < (1 << 24) - 64) {
        rc = alloc_folded(*snap, pairs[0], folded);  // (the canonicalising kernel below writes it)
        if (rc != FPE_OK) return rc;
    }
    for (int l = 0; l < 2; ++l) {
        uint32_t* planeWords = (l == 0 && folded) ? folded->d_words : nullptr;
        if (canonical && !planeWords) {
            FPE_HIP(hipMemcpyAsync(dst[l], src[l], n * sizeof(float),
                                   srcOnDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
        } else {
            const float* dsrc = src[l];
            if (!srcOnDevice) {
                FPE_HIP(hipMemcpyAsync(staging, src[l], n * sizeof(float), hipMemcpyHostToDevice, stream));
                dsrc = staging;
            }
            FPE_HIP(fpe::launch_canonicalise(dsrc, dst[l], desc->rows, desc->cols, desc->start_index[0], desc->start_index[1],
                                             desc->storage_order, stream, planeWords, planeWords ? folded->thrD : 0.0f,
                                             planeWords ? folded->thrC : 0.0f));
        }
        if (!srcOnDevice) FPE_HIP(hipStreamSynchronize(stream));  // host buffers may be freed on return
    }
    // consumers on other streams wait for this event before their first kernel (device-source uploads are
    // asynchronous; host-source uploads have been synchronised above, the event is then already complete)
    FPE_HIP(hipEventCreateWithFlags(&snap->ready, hipEventDisableTiming));
    FPE_HIP(hipEventRecord(snap->ready, stream));
    if (folded) {
        rc = folded_ready(*snap, folded, stream);
        if (rc != FPE_OK) return rc;
    }
    rc = build_carried_planes(*snap, pairs, folded ? 1 : 0, stream, false);
    if (rc != FPE_OK) return rc;
    return install_snapshot(h, snap, !srcOnDevice, stream);
}

// The patches of an update into its argument block.  Device form: the caller's arrays as they are.  Host form: packed row-major
// into a call context's pinned arena (their strides resolved here), ONE host-to-device copy queued on the context's stream, which
// becomes `stream`; the caller synchronises it and clears lease->ctx->inFlight.  elevationOnly: the patches of fpe_update_elevation*
// (one layer; the kernel's traversability pointer stays null).
int stage_update_patches(fpe_engine* h, const fpe_map_update* u, bool srcOnDevice, bool elevationOnly, fpe::MapUpdateArgs& a,
                         std::unique_ptr<CtxLease>& lease, hipStream_t& stream) {
    const int nl = elevationOnly ? 1 : 2;
    if (srcOnDevice) {
        for (int k = 0; k < u->n_patches; ++k) {
            const fpe_map_patch& p = u->patch[k];
            a.patch[k] = fpe::MapUpdatePatch{p.row0, p.col0, p.n_rows, p.n_cols, reinterpret_cast<const uint32_t*>(p.traversability),
                                             reinterpret_cast<const uint32_t*>(p.elevation), p.row_stride, p.col_stride};
        }
        return FPE_OK;
    }
    lease.reset(new CtxLease(h->ctxPool));
    CallCtx& cx = *lease->ctx;
    size_t cells = 0;
    for (int k = 0; k < u->n_patches; ++k) cells += static_cast<size_t>(u->patch[k].n_rows) * u->patch[k].n_cols;
    const size_t bytes = nl * cells * sizeof(float);
    FPE_HIP(cx.reserve(bytes));
    stream = cx.stream;
    float* hp = reinterpret_cast<float*>(cx.pinned);
    size_t off = 0;
    for (int k = 0; k < u->n_patches; ++k) {
        const fpe_map_patch& p = u->patch[k];
        const size_t pn = static_cast<size_t>(p.n_rows) * p.n_cols;
        const float* src[2] = {elevationOnly ? p.elevation : p.traversability, p.elevation};
        for (int l = 0; l < nl; ++l)
            for (int r = 0; r < p.n_rows; ++r) {
                float* row = hp + off + l * pn + static_cast<size_t>(r) * p.n_cols;
                if (p.col_stride == 1) std::memcpy(row, src[l] + r * p.row_stride, static_cast<size_t>(p.n_cols) * sizeof(float));
                else
                    for (int c = 0; c < p.n_cols; ++c) row[c] = src[l][r * p.row_stride + c * p.col_stride];
            }
        const uint32_t* dp = reinterpret_cast<const uint32_t*>(cx.dev) + off;
        a.patch[k] = fpe::MapUpdatePatch{p.row0, p.col0, p.n_rows, p.n_cols, elevationOnly ? nullptr : dp, elevationOnly ? dp : dp + pn, p.n_cols, 1};
        off += nl * pn;
    }
    cx.inFlight = true;
    if (bytes) FPE_HIP(hipMemcpyAsync(cx.dev, cx.pinned, bytes, hipMemcpyHostToDevice, stream));
    return FPE_OK;
}

// ---- what fpe_update_map* and fpe_update_elevation* share: an incremental update from its entry to its composing kernel's
// arguments (update_open) and from the finished layers to the installed snapshot (update_close) -------------------------------------
struct UpdateCall {
    std::unique_lock<std::mutex> serial;  // h->updateMu, for the whole call
    // (declared ahead of the lease: on an early exit the lease waits for its stream BEFORE the snapshots are released, as in HostCall)
    CallPlan baseRef;
    std::shared_ptr<MapSnapshot> snap;
    std::unique_ptr<CtxLease> lease;
    fpe::MapUpdateArgs a;
    hipStream_t stream = nullptr;
    bool srcOnDevice = false;
};
// The snapshot current at entry as the base, check(base geometry, &why) — the call's refusals —, the new snapshot, map_update_kernel's
// arguments but for the pairs, the patches staged (host form: ONE host-to-device copy on the call context's stream, which becomes
// uc.stream), and that stream behind the base's upload.
template <class Check>
int update_open(fpe_engine* h, const fpe_map_update* u, bool srcOnDevice, bool elevationOnly, hipStream_t stream, UpdateCall& uc, Check check) {
    if (!h || !u) return fail(FPE_E_INVALID_ARG, "null handle or update");
    uc.serial = std::unique_lock<std::mutex>(h->updateMu);
    std::shared_ptr<MapSnapshot>& base = uc.baseRef.snap;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        base = h->map;
    }
    if (!base) return fail(FPE_E_NO_MAP, "no map uploaded");
    const int rows = base->g.rows, cols = base->g.cols;
    const char* why = "";
    int rc = check(base->g, &why);
    if (rc != FPE_OK) return fail(rc, why);
    FPE_HIP(hipSetDevice(h->device));
    rc = new_snapshot(h, rows, cols, base->g.res, u->position[0], u->position[1], uc.snap);
    if (rc != FPE_OK) return rc;

    fpe::MapUpdateArgs& a = uc.a;
    std::memset(&a, 0, sizeof(a));
    a.baseTrav = reinterpret_cast<const uint32_t*>(base->d_trav);
    a.baseElev = reinterpret_cast<const uint32_t*>(base->d_elev);
    a.dstTrav = reinterpret_cast<uint32_t*>(uc.snap->d_trav);
    a.dstElev = reinterpret_cast<uint32_t*>(uc.snap->d_elev);
    a.rows = rows;
    a.cols = cols;
    a.sr = std::max(-rows, std::min(rows, u->shift[0]));  // beyond +-rows nothing is carried either way
    a.sc = std::max(-cols, std::min(cols, u->shift[1]));
    a.nPatches = u->n_patches;
    uc.stream = stream;
    uc.srcOnDevice = srcOnDevice;
    rc = stage_update_patches(h, u, srcOnDevice, elevationOnly, a, uc.lease, uc.stream);
    if (rc != FPE_OK) return rc;
    FPE_HIP(base->wait_ready(uc.stream));  // the update's stream behind the base's upload
    // the device form reads the base asynchronously and keeps no reference past this call: the base counts as read by an
    // asynchronous launch, so its buffers (and, through ~MapSnapshot, its planes) are recycled only behind a device synchronisation
    if (srcOnDevice) mark_async_launch(uc.baseRef);
    return FPE_OK;
}
// Behind the kernels that wrote the new snapshot's layers: its ready event, planes() — the carried pairs' planes into the snapshot's
// sets —, the host form's synchronisation, and the snapshot becomes the engine's current one.
template <class Planes>
int update_close(fpe_engine* h, UpdateCall& uc, Planes planes) {
    FPE_HIP(hipEventCreateWithFlags(&uc.snap->ready, hipEventDisableTiming));
    FPE_HIP(hipEventRecord(uc.snap->ready, uc.stream));
    const int rc = planes();
    if (rc != FPE_OK) return rc;
    if (!uc.srcOnDevice) {  // host sources may be freed on return — and the arena goes back to the pool
        FPE_HIP(hipStreamSynchronize(uc.stream));
        uc.lease->ctx->inFlight = false;
    }
    return install_snapshot(h, uc.snap, !uc.srcOnDevice, uc.stream);
}

// fpe_update_map*: the snapshot current at entry shifted by whole cells, cleared where nothing is carried, the patches written over
// that (include/fpe.h) — one launch of map_update_kernel, which also writes the planes of every pair the base was planned with.
// Host form: the patches packed row-major into the call context's pinned arena (their strides resolved here), ONE host-to-device
// copy, the kernel on the context's stream, one synchronisation.  Device form: the caller's patch arrays as they are, on `stream`.
int update_common(fpe_engine* h, const fpe_map_update* u, bool srcOnDevice, hipStream_t stream) {
    UpdateCall uc;
    int rc = update_open(h, u, srcOnDevice, false, stream, uc,
                         [&](const fpe::MapGeom& g, const char** why) { return fpe::check_map_update(g.rows, g.cols, u, false, why); });
    if (rc != FPE_OK) return rc;
    fpe::MapUpdateArgs& a = uc.a;
    const std::vector<std::pair<float, float>> pairs = carried_pairs(uc.baseRef.snap);
    std::vector<std::shared_ptr<MaskSet>> folded(pairs.size());
    a.nPairs = static_cast<int32_t>(std::min<size_t>(pairs.size(), fpe::kUpdateMaxPairs));
    for (int k = 0; k < a.nPairs; ++k) {
        rc = alloc_folded(*uc.snap, pairs[static_cast<size_t>(k)], folded[static_cast<size_t>(k)]);
        if (rc != FPE_OK) return rc;
        a.pair[k] = fpe::MapUpdatePair{reinterpret_cast<uint4*>(folded[static_cast<size_t>(k)]->d_words), pairs[static_cast<size_t>(k)].first,
                                       pairs[static_cast<size_t>(k)].second};
    }
    FPE_HIP(fpe::launch_map_update(a, uc.stream));
    return update_close(h, uc, [&]() {
        for (int k = 0; k < a.nPairs; ++k) {
            const int rk = folded_ready(*uc.snap, folded[static_cast<size_t>(k)], uc.stream);
            if (rk != FPE_OK) return rk;
        }
        return static_cast<int>(FPE_OK);
    });
}

// The producer's chain on `stream` for the map of geometry g, as `rt` decided it (ONE filter_route per API call).
//   travOnly (rt.travOnly): the two-launch chain that stores step_height — into a slot of fpe_engine::filterSlots, under filterMu —
//     and traversability, straight into d_trav: over the whole map or, with `region`, over its tiles;
//   else: the full chain through eight layers — the caller's (d_layers) or pooled ones (taken into `pooled` here; cleanOnly as in
//     alloc_units) — and, where d_trav is given and is not the layers' own traversability, the device-to-device copy into it.
int run_filter_chain(fpe_engine* h, const fpe::MapGeom& g, const fpe::FilterConsts& fc, const fpe::FilterRoute& rt, const fpe::FilterRegion* region, bool travOnly,
                     const float* d_elev, float* d_trav, float* d_layers, PooledBuf& pooled, bool cleanOnly, hipStream_t stream) {
    const size_t n = static_cast<size_t>(g.rows) * g.cols;
    if (travOnly) {
        // the lock is held until the chain is QUEUED and its event recorded (see fpe_engine::filterSlots)
        std::lock_guard<std::mutex> lk(h->filterMu);
        fpe_engine::FilterSlot* slot = nullptr;
        const int rc = filter_slot_take(h, n, stream, slot);
        if (rc != FPE_OK) return rc;
        const fpe::FilterLayers L{nullptr, nullptr, nullptr, nullptr, slot->buf, nullptr, nullptr, d_trav};
        const hipError_t e = fpe::launch_filters(g, fc, rt, d_elev, L, true, region, stream);
        const hipError_t f = filter_slot_done(h, slot, stream);  // also behind a chain that failed half-way
        FPE_HIP(e);
        FPE_HIP(f);
        return FPE_OK;
    }
    if (!d_layers) {
        FPE_HIP(pooled.take(8 * n, cleanOnly));
        d_layers = pooled.p;
    }
    const fpe::FilterLayers L{d_layers, d_layers + n, d_layers + 2 * n, d_layers + 3 * n, d_layers + 4 * n, d_layers + 5 * n,
                              d_layers + 6 * n, d_layers + 7 * n};
    FPE_HIP(fpe::launch_filters(g, fc, rt, d_elev, L, false, nullptr, stream));
    if (d_trav && d_trav != L.trav) FPE_HIP(hipMemcpyAsync(d_trav, L.trav, n * sizeof(float), hipMemcpyDeviceToDevice, stream));
    return FPE_OK;
}

// fpe_update_elevation*: fpe_update_map's composition with elevation-only patches (the traversability layer is carried or cleared),
// then the producer's chain over the dirty tiles straight into the new snapshot's traversability layer — region launches (route 0)
// or, where the chain is not the two-launch traversability-only one, the full chain over the whole composed map (route 1) — then the
// planes of the base's threshold pairs from the finished layer (launch_build_bitmap: one pass over T* per pair; the planes cannot
// ride in map_update_kernel here, the chain writes T* behind it).  One stream: compose -> step heights -> fused -> planes.
int update_elevation_common(fpe_engine* h, const fpe_filter_params* fp, const fpe_map_update* u, fpe_elevation_update_info* info, bool srcOnDevice,
                            hipStream_t stream) {
    UpdateCall uc;
    fpe::ElevationUpdatePlan plan;
    int rc = update_open(h, u, srcOnDevice, true, stream, uc, [&](const fpe::MapGeom& g, const char** why) {
        return fpe::plan_elevation_update(g.rows, g.cols, g.res, fp, u, plan, why);
    });
    if (rc != FPE_OK) return rc;
    MapSnapshot& snap = *uc.snap;
    // the new snapshot's own layers are written asynchronously from here on: should a later step fail, they go back dirty
    struct DirtyOnExit {
        MapSnapshot* s;
        ~DirtyOnExit() {
            if (s) s->note_async_use();
        }
    } dirtyOnExit{srcOnDevice ? &snap : nullptr};
    FPE_HIP(fpe::launch_map_update(uc.a, uc.stream));  // (nPairs 0: the planes follow the chain)

    // pooled scratch of the full chain with intermediate layers (route 1 where the chain is not the traversability-only one);
    // device form: never a device synchronisation
    PooledBuf scratch{h->pool, true};
    const bool region = plan.info.route == 0;
    rc = run_filter_chain(h, plan.g, plan.fc, plan.rt, region ? &plan.region : nullptr, region || plan.rt.travOnly, snap.d_elev, snap.d_trav, nullptr, scratch,
                          srcOnDevice, uc.stream);
    if (rc != FPE_OK) return rc;
    rc = update_close(h, uc, [&]() { return build_carried_planes(snap, carried_pairs(uc.baseRef.snap), 0, uc.stream, srcOnDevice); });
    if (rc != FPE_OK) return rc;
    dirtyOnExit.s = nullptr;
    if (info) *info = plan.info;
    return FPE_OK;
}

// fpe_read_map_layers*: the canonical layers of the snapshot current at entry, copied out bit for bit.
int read_layers_common(fpe_engine* h, float* trav, float* elev, bool onDevice, hipStream_t stream) {
    if (!h || (!trav && !elev)) return fail(FPE_E_INVALID_ARG, "null handle, or no layer requested");
    std::shared_ptr<MapSnapshot> snap;  // (ahead of the lease: on an early exit the lease waits for its stream first)
    {
        std::lock_guard<std::mutex> lk(h->mu);
        snap = h->map;
    }
    if (!snap) return fail(FPE_E_NO_MAP, "no map uploaded");
    FPE_HIP(hipSetDevice(h->device));
    const size_t bytes = snap->n * sizeof(float);
    if (onDevice) {
        FPE_HIP(snap->wait_ready(stream));
        snap->note_async_use();  // read without the host waiting: the layers are recycled only behind a device synchronisation
        if (trav) FPE_HIP(hipMemcpyAsync(trav, snap->d_trav, bytes, hipMemcpyDeviceToDevice, stream));
        if (elev) FPE_HIP(hipMemcpyAsync(elev, snap->d_elev, bytes, hipMemcpyDeviceToDevice, stream));
        return FPE_OK;
    }
    CtxLease lease(h->ctxPool);
    CallCtx& cx = *lease.ctx;
    FPE_HIP(cx.reserve(0));
    FPE_HIP(snap->wait_ready(cx.stream));
    cx.inFlight = true;
    if (trav) FPE_HIP(hipMemcpyAsync(trav, snap->d_trav, bytes, hipMemcpyDeviceToHost, cx.stream));
    if (elev) FPE_HIP(hipMemcpyAsync(elev, snap->d_elev, bytes, hipMemcpyDeviceToHost, cx.stream));
    FPE_HIP(hipStreamSynchronize(cx.stream));
    cx.inFlight = false;
    return FPE_OK;
}

}  // namespace

extern "C" {

int fpe_abi_version(void) { return FPE_ABI_VERSION; }
const char* fpe_version(void) { return "fpe 0.5.0 (gfx950, wave64; bit-window plan kernels on tiled planes: 8 lanes per leg and two poses per wavefront, one wavefront per pose for large windows; opt track with a build-defined optimiser)"; }

const char* fpe_last_error(fpe_handle) { return g_err.c_str(); }

int fpe_create(int device_id, fpe_handle* out) {
    if (!out) return fail(FPE_E_INVALID_ARG, "null out handle");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) return fail(FPE_E_NO_DEVICE, "no HIP device visible");
    if (device_id < 0 || device_id >= count) return fail(FPE_E_INVALID_ARG, "device id out of range");
    FPE_HIP(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    FPE_HIP(hipGetDeviceProperties(&prop, device_id));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(FPE_E_NO_DEVICE, std::string("device is not gfx950: ") + prop.gcnArchName);
    fpe_engine* h = new (std::nothrow) fpe_engine();
    if (!h) return fail(FPE_E_NOMEM, "out of host memory");
    h->device = device_id;
    // tuning defaults: the environment is read HERE, once per engine — never in the per-call path
    if (const char* v = std::getenv("FPE_PLAN_GROUP")) h->tuning.planGroup = std::atoi(v);
    if (std::getenv("FPE_LITERAL_DISCS")) h->tuning.literalDiscs = 1;
    if (std::getenv("FPE_NO_MID_VARIANT")) h->tuning.noMidVariant = 1;
    if (std::getenv("FPE_NO_BITS")) h->tuning.noBits = 1;
    fpe::SpiralTable t;
    fpe::build_spiral_table(fpe::kMaxRings, t);
    h->maxRing = t.maxRing;
    h->ringStart = t.ringStart;
    const size_t n = t.di.size();
    auto cleanup = [&]() { fpe_destroy(h); };
#define FPE_HIP_C(call)                       \
    do {                                      \
        hipError_t e_ = (call);               \
        if (e_ != hipSuccess) {               \
            cleanup();                        \
            return fail_hip(e_, #call);       \
        }                                     \
    } while (0)
    FPE_HIP_C(hipMalloc(reinterpret_cast<void**>(&h->d_di), n * sizeof(int16_t)));
    FPE_HIP_C(hipMalloc(reinterpret_cast<void**>(&h->d_dj), n * sizeof(int16_t)));
    FPE_HIP_C(hipMalloc(reinterpret_cast<void**>(&h->d_ring), n * sizeof(uint8_t)));
    FPE_HIP_C(hipMalloc(reinterpret_cast<void**>(&h->d_ringStart), t.ringStart.size() * sizeof(int32_t)));
    FPE_HIP_C(hipMemcpy(h->d_di, t.di.data(), n * sizeof(int16_t), hipMemcpyHostToDevice));
    FPE_HIP_C(hipMemcpy(h->d_dj, t.dj.data(), n * sizeof(int16_t), hipMemcpyHostToDevice));
    FPE_HIP_C(hipMemcpy(h->d_ring, t.ring.data(), n * sizeof(uint8_t), hipMemcpyHostToDevice));
    FPE_HIP_C(hipMemcpy(h->d_ringStart, t.ringStart.data(), t.ringStart.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    {
        std::vector<uint32_t> packed(((n + 31) / 32 + 1) * 32, 255u << 16);  // SpiralLut::packed
        for (size_t k = 0; k < n; ++k)
            packed[k] = (static_cast<uint32_t>(t.di[k]) & 0xFFu) | ((static_cast<uint32_t>(t.dj[k]) & 0xFFu) << 8) | (static_cast<uint32_t>(t.ring[k]) << 16);
        FPE_HIP_C(hipMalloc(reinterpret_cast<void**>(&h->d_packed), packed.size() * sizeof(uint32_t)));
        FPE_HIP_C(hipMemcpy(h->d_packed, packed.data(), packed.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        // SpiralLut::fast16: the first sixteen ranks by row (they all lie within two cells of the centre: rings 0-2)
        uint32_t fast[fpe::kFast16Words] = {0};
        for (int r = 0; r < 5; ++r) fast[r] = 0x1FFFFFFu;  // five 5-bit fields, 31 = none
        unsigned long long tdi = 0ull, tdj = 0ull;
        bool fastOk = n >= 16;
        for (size_t q = 0; q < 16 && fastOk; ++q) {
            const int di = t.di[q], dj = t.dj[q];
            if (di < -2 || di > 2 || dj < -2 || dj > 2) {
                fastOk = false;
                break;
            }
            uint32_t& w = fast[di + 2];
            w = (w & ~(31u << (5 * (dj + 2)))) | (static_cast<uint32_t>(q) << (5 * (dj + 2)));
            tdi |= static_cast<unsigned long long>(di + 2) << (4 * q);
            tdj |= static_cast<unsigned long long>(dj + 2) << (4 * q);
        }
        if (!fastOk) {
            cleanup();
            return fail(FPE_E_HIP, "spiral table: the first sixteen ranks do not lie within two cells of the centre");
        }
        fast[6] = static_cast<uint32_t>(tdi);
        fast[7] = static_cast<uint32_t>(tdi >> 32);
        fast[8] = static_cast<uint32_t>(tdj);
        fast[9] = static_cast<uint32_t>(tdj >> 32);
        FPE_HIP_C(hipMalloc(reinterpret_cast<void**>(&h->d_fast16), sizeof(fast)));
        FPE_HIP_C(hipMemcpy(h->d_fast16, fast, sizeof(fast), hipMemcpyHostToDevice));
    }
    // every kernel may use the whole 160 KiB of LDS: set once per process and device, never lowered again (a
    // second engine on the same device sets the same value)
    FPE_HIP_C(fpe::set_max_lds(kMaxLdsBytes, kMaxLdsBytes));
    FPE_HIP_C(fpe::set_max_lds_rank());
#undef FPE_HIP_C
    *out = h;
    return FPE_OK;
}

int fpe_destroy(fpe_handle h) {
    if (!h) return FPE_OK;
    (void)hipSetDevice(h->device);
    (void)hipDeviceSynchronize();
    if (h->d_di) (void)hipFree(h->d_di);
    if (h->d_dj) (void)hipFree(h->d_dj);
    if (h->d_ring) (void)hipFree(h->d_ring);
    if (h->d_ringStart) (void)hipFree(h->d_ringStart);
    if (h->d_packed) (void)hipFree(h->d_packed);
    if (h->d_fast16) (void)hipFree(h->d_fast16);
    for (auto& fs : h->filterSlots) {
        if (fs.buf) (void)hipFree(fs.buf);
        if (fs.done) (void)hipEventDestroy(fs.done);
    }
    h->map.reset();
    delete h;
    return FPE_OK;
}

int fpe_set_tuning(fpe_handle h, const char* key, int32_t value) {
    if (!h || !key) return fail(FPE_E_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    const std::string k(key);
    if (k == "plan_group") h->tuning.planGroup = value;
    else if (k == "literal_discs") h->tuning.literalDiscs = value ? 1 : 0;
    else if (k == "no_mid_variant") h->tuning.noMidVariant = value ? 1 : 0;
    else if (k == "no_bits") h->tuning.noBits = value ? 1 : 0;
    else if (k == "service_opt_gate") {
        if (value < 0 || value > 2) return fail(FPE_E_INVALID_ARG, "service_opt_gate is 0 (exact gates only), 1 (advisory) or 2 (enforce)");
        h->tuning.serviceOptGate = value;
    } else if (k == "beam_check_waves") {
        if (value != 0 && value != 1 && value != 4) return fail(FPE_E_INVALID_ARG, "beam_check_waves is 0 (automatic), 1 or 4");
        h->tuning.beamCheckWaves = value;
    } else if (k == "scan_merge") {
        if (value < 0 || value > 2) return fail(FPE_E_INVALID_ARG, "scan_merge is 0 (the engine's choice), 1 (plain) or 2 (merged)");
        h->tuning.scanMerge = value;
    } else if (k == "scan_clear_form") {
        if (value < 0 || value > 2) return fail(FPE_E_INVALID_ARG, "scan_clear_form is 0 (the engine's choice), 1 (a lane per ray) or 2 (a group per ray)");
        h->tuning.scanClearForm = value;
    } else if (k == "scan_clear_group") {
        if (value != 0 && value != 16 && value != 32 && value != 64) return fail(FPE_E_INVALID_ARG, "scan_clear_group is 0 (the engine's choice), 16, 32 or 64");
        h->tuning.scanClearGroup = value;
    } else if (k == "scan_close_form") {
        if (value < 0 || value > 2) return fail(FPE_E_INVALID_ARG, "scan_close_form is 0 (the engine's choice), 1 (direct) or 2 (tiled)");
        h->tuning.scanCloseForm = value;
    } else if (k == "service_overlap") h->tuning.serviceOverlap = value ? 1 : 0;
    else if (k == "service_poll") h->tuning.servicePoll = value ? 1 : 0;
    else if (k == "service_cycle0_gate_only") h->tuning.serviceOptGate = value ? 0 : 2;  // (older name)
    else return fail(FPE_E_INVALID_ARG, "unknown tuning key: " + k);
    return FPE_OK;
}

static int describe_plan(fpe_handle h, const fpe_params* params, char* buf, int32_t n, fpe::PlanForm form) {
    if (!h || !params || !buf || n <= 0) return fail(FPE_E_INVALID_ARG, "null argument");
    std::shared_ptr<MapSnapshot> snap;
    fpe::Tuning tuning;
    float maxRadius;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        snap = h->map;
        tuning = h->tuning;
        maxRadius = std::max(params->searchRadius, h->maxLegSearchRadius);
    }
    if (!snap) return fail(FPE_E_NO_MAP, "no map uploaded");
    fpe::PlanConsts pc;
    fpe::derive_constants(*params, snap->g, maxRadius, tuning, pc);
    // (the family-level part of the selection: no batch, no products)
    fpe::describe_plan_kernel(fpe::select_plan_kernel(pc, snap->g, fpe::bits_supported(pc, snap->g), 0, 0, form), buf, static_cast<size_t>(n));
    return FPE_OK;
}
int fpe_describe_plan(fpe_handle h, const fpe_params* params, char* buf, int32_t n) { return describe_plan(h, params, buf, n, fpe::PlanForm::Plain); }
int fpe_describe_plan_strides(fpe_handle h, const fpe_params* params, char* buf, int32_t n) { return describe_plan(h, params, buf, n, fpe::PlanForm::Stride); }
int fpe_describe_plan_resume(fpe_handle h, const fpe_params* params, char* buf, int32_t n) { return describe_plan(h, params, buf, n, fpe::PlanForm::Resume); }

int fpe_set_max_leg_search_radius(fpe_handle h, float radius) {
    if (!h || !(radius >= 0.0f) || !std::isfinite(radius)) return fail(FPE_E_INVALID_ARG, "bad radius");
    std::lock_guard<std::mutex> lk(h->mu);
    h->maxLegSearchRadius = radius;
    return FPE_OK;
}

int fpe_upload_map(fpe_handle h, const fpe_map_desc* desc, const float* traversability, const float* elevation) {
    return upload_common(h, desc, traversability, elevation, false, nullptr);
}

int fpe_upload_map_device(fpe_handle h, const fpe_map_desc* desc, const float* d_traversability,
                          const float* d_elevation, void* stream) {
    return upload_common(h, desc, d_traversability, d_elevation, true, static_cast<hipStream_t>(stream));
}

int fpe_update_map(fpe_handle h, const fpe_map_update* u) { return update_common(h, u, false, nullptr); }

int fpe_update_map_device(fpe_handle h, const fpe_map_update* u, void* stream) {
    return update_common(h, u, true, static_cast<hipStream_t>(stream));
}

int fpe_update_elevation(fpe_handle h, const fpe_filter_params* fp, const fpe_map_update* u, fpe_elevation_update_info* info) {
    return update_elevation_common(h, fp, u, info, false, nullptr);
}

int fpe_update_elevation_device(fpe_handle h, const fpe_filter_params* fp, const fpe_map_update* u, fpe_elevation_update_info* info, void* stream) {
    return update_elevation_common(h, fp, u, info, true, static_cast<hipStream_t>(stream));
}

int fpe_read_map_layers(fpe_handle h, float* traversability, float* elevation) { return read_layers_common(h, traversability, elevation, false, nullptr); }

int fpe_read_map_layers_device(fpe_handle h, float* d_traversability, float* d_elevation, void* stream) {
    return read_layers_common(h, d_traversability, d_elevation, true, static_cast<hipStream_t>(stream));
}

int fpe_filter_params_defaults(fpe_filter_params* out) {
    if (!out) return fail(FPE_E_INVALID_ARG, "null out");
    fpe::filter_params_defaults(*out);
    return FPE_OK;
}

namespace {
int filters_common(fpe_engine* h, const fpe_map_desc* desc, const fpe_filter_params* fp, const float* elev, bool onDevice,
                   float* trav, float* layers, hipStream_t stream) {
    if (!h || !fp || !elev || !trav) return fail(FPE_E_INVALID_ARG, "null argument");
    int rc = check_desc(desc);
    if (rc != FPE_OK) return rc;
    fpe::FilterConsts fc;
    if (fpe::filter_consts(*fp, fc) != FPE_OK) return fail(FPE_E_INVALID_ARG, fpe::kBadFilterParams);
    const fpe::MapGeom g = fpe::make_geom(desc->rows, desc->cols, desc->resolution, desc->position[0], desc->position[1]);
    if (!fpe::filters_supported(fc, g)) return fail(FPE_E_UNSUPPORTED, "filter radius spans more cells than the stencil tables hold");
    const fpe::FilterRoute rt = fpe::filter_route(fc, g);
    FPE_HIP(hipSetDevice(h->device));
    const size_t n = static_cast<size_t>(desc->rows) * desc->cols;
    const bool canonical = desc->storage_order == 1 && desc->start_index[0] == 0 && desc->start_index[1] == 0;
    // pooled scratch: the canonical elevation (when the source is a host buffer or in message layout), its staging copy, a host
    // caller's traversability and the eight layers
    // (handed back marked dirty: the next taker synchronises the device before reuse, BufferPool)
    PooledBuf canon{h->pool, true}, staging{h->pool, true}, travBuf{h->pool, true}, layerBuf{h->pool, true};
    const float* d_elev = elev;
    if (!onDevice || !canonical) {
        FPE_HIP(canon.take(n));
        const float* dsrc = elev;
        if (!onDevice) {
            float* stage = canon.p;
            if (!canonical) {
                FPE_HIP(staging.take(n));
                stage = staging.p;
            }
            FPE_HIP(hipMemcpyAsync(stage, elev, n * sizeof(float), hipMemcpyHostToDevice, stream));
            dsrc = stage;
        }
        if (!canonical)
            FPE_HIP(fpe::launch_canonicalise(dsrc, canon.p, desc->rows, desc->cols, desc->start_index[0], desc->start_index[1],
                                             desc->storage_order, stream));
        d_elev = canon.p;
    }
    // Nobody asked for the intermediate layers (device caller without a layer buffer, host caller without `layers`): the
    // two-launch chain that stores step_height and traversability only, traversability straight into the caller's buffer
    // when it is a device buffer.
    // (not when the caller's traversability buffer IS — or overlaps — the elevation buffer: the fused launch writes traversability
    // tile by tile while its neighbours still read their halos; the layer-buffer path below writes scratch and copies afterwards)
    const bool inPlace = onDevice && trav < elev + n && elev < trav + n;
    const bool travOnly = !layers && !inPlace && rt.travOnly;
    float* d_trav = onDevice ? trav : nullptr;
    if (travOnly && !onDevice) {
        FPE_HIP(travBuf.take(n));
        d_trav = travBuf.p;
    }
    rc = run_filter_chain(h, g, fc, rt, nullptr, travOnly, d_elev, d_trav, onDevice ? layers : nullptr, layerBuf, false, stream);
    if (rc != FPE_OK) return rc;
    if (!onDevice) {
        FPE_HIP(hipMemcpyAsync(trav, travOnly ? d_trav : layerBuf.p + 7 * n, n * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (layers) FPE_HIP(hipMemcpyAsync(layers, layerBuf.p, 8 * n * sizeof(float), hipMemcpyDeviceToHost, stream));
        FPE_HIP(hipStreamSynchronize(stream));
    }
    return FPE_OK;
}
}  // namespace

int fpe_traversability(fpe_handle h, const fpe_map_desc* desc, const fpe_filter_params* fp, const float* elevation,
                       float* traversability, float* layers) {
    return filters_common(h, desc, fp, elevation, false, traversability, layers, nullptr);
}

int fpe_traversability_device(fpe_handle h, const fpe_map_desc* desc, const fpe_filter_params* fp, const float* d_elevation,
                              float* d_traversability, float* d_layers, void* stream) {
    return filters_common(h, desc, fp, d_elevation, true, d_traversability, d_layers, static_cast<hipStream_t>(stream));
}

int fpe_map_info(fpe_handle h, fpe_map_desc* out) {
    if (!h || !out) return fail(FPE_E_INVALID_ARG, "null argument");
    std::shared_ptr<MapSnapshot> snap;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        snap = h->map;
    }
    if (!snap) return fail(FPE_E_NO_MAP, "no map uploaded");
    out->rows = snap->g.rows;
    out->cols = snap->g.cols;
    out->resolution = snap->g.res;
    out->position[0] = snap->g.posX;
    out->position[1] = snap->g.posY;
    out->start_index[0] = out->start_index[1] = 0;
    out->storage_order = 1;
    return FPE_OK;
}

// One chained-plan launch on `stream`: the bit-window kernels when the snapshot's bit planes apply, else the direct ones.
// chain: the optional arrays of fpe_plan_strides* / fpe_plan_rank_strides* (the stride form) and fpe_plan_resume* (the resume form,
// which exists where the stride form does).
static int check_strides_launchable(const CallPlan& cp, fpe::PlanForm form) {
    if (form != fpe::PlanForm::Plain && fpe::select_plan_kernel(cp.pc, cp.snap->g, cp.useBits, 0, 0, form).family == fpe::PlanFamily::None)
        return fail(FPE_E_UNSUPPORTED, form == fpe::PlanForm::Resume ? "resumable plans: no resume kernel for a forced plan_group of 4, 16 or 64"
                                                                    : "per-pose strides: no stride kernel for a forced plan_group of 4, 16 or 64");
    return FPE_OK;
}
// stance and pose_status are products of a start, not of a continuation (include/fpe.h)
static int check_resumed_products(const fpe_plan_state* stateIn, const fpe_plan_out& out) {
    if (stateIn && (out.stance || out.pose_status))
        return fail(FPE_E_INVALID_ARG, "a resumed plan (state_in given) has no stance and no pose_status");
    return FPE_OK;
}
static int launch_plan(fpe_engine* h, const CallPlan& cp, const fpe_pose* d_poses, int32_t B, int32_t n_cycles,
                       const fpe_plan_out& d_out, hipStream_t stream, const fpe::PlanChain& chain = {}) {
    int rc = check_packed_fits(cp, d_out.selected_packed != nullptr);
    if (rc != FPE_OK) return rc;
    rc = check_strides_launchable(cp, chain.form());
    if (rc != FPE_OK) return rc;
    FPE_HIP(fpe::launch_plan(dev_map(*cp.snap), cp.useBits ? &cp.bits : nullptr, cp.pc, h->lut(), d_poses, B, n_cycles, d_out, chain, stream));
    return FPE_OK;
}

int fpe_plan_device(fpe_handle h, const fpe_params* params, const fpe_pose* d_poses, int32_t B, int32_t n_cycles,
                    const fpe_plan_out* d_out, void* stream) {
    return fpe_plan_strides_device(h, params, d_poses, nullptr, B, n_cycles, d_out, stream);
}

int fpe_plan_strides_device(fpe_handle h, const fpe_params* params, const fpe_pose* d_poses, const fpe_stride* d_strides, int32_t B,
                            int32_t n_cycles, const fpe_plan_out* d_out, void* stream) {
    return fpe_plan_resume_device(h, params, d_poses, d_strides, nullptr, B, n_cycles, d_out, nullptr, stream);
}

int fpe_plan_resume_device(fpe_handle h, const fpe_params* params, const fpe_pose* d_poses, const fpe_stride* d_strides,
                           const fpe_plan_state* d_state_in, int32_t B, int32_t n_cycles, const fpe_plan_out* d_out,
                           fpe_plan_state* d_state_out, void* stream) {
    if (!d_poses || !d_out) return fail(FPE_E_INVALID_ARG, "null argument");
    if (B <= 0 || n_cycles <= 0 || n_cycles > 255) return fail(FPE_E_INVALID_ARG, "B and n_cycles must be in [1, ..] / [1, 255]");
    int rc = check_resumed_products(d_state_in, *d_out);
    if (rc != FPE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    CallPlan cp;
    rc = prepare_call(h, params, 0.0f, cp, st, true);
    if (rc != FPE_OK) return rc;
    const fpe::PlanChain chain{d_strides, d_state_in, d_state_out};
    rc = check_strides_launchable(cp, chain.form());  // (a refusal queues nothing: ahead of the async mark)
    if (rc != FPE_OK) return rc;
    rc = check_packed_fits(cp, d_out->selected_packed != nullptr);
    if (rc != FPE_OK) return rc;
    mark_async_launch(cp);
    return launch_plan(h, cp, d_poses, B, n_cycles, *d_out, st, chain);
}

namespace {
// Constants of the opt track for this map, checked (fpe_host.cpp::derive_opt_constants).
int prepare_opt(const fpe_params* params, const fpe_opt_params* opt, const CallPlan& cp, float maxRadius, fpe::OptConsts& oc) {
    fpe_opt_params yaml;
    if (!opt) {
        fpe_opt_params_yaml(&yaml);
        opt = &yaml;
    }
    const int rc = fpe::derive_opt_constants(*params, *opt, cp.snap->g, cp.pc, oc);
    if (rc != FPE_OK) return fail(rc, "opt parameters: weights / scales / tolerance must be finite");
    // checkFootholdUseCentroidMethod on the gait-cycle submap keeps its blocked-row mask in 128 bits
    const double rows = 2.0 * static_cast<double>(std::max(maxRadius, params->searchRadius)) / cp.snap->g.res + 3.0;
    if (rows > 128.0) return fail(FPE_E_UNSUPPORTED, "opt track: the foot search rectangle spans more than 128 rows");
    return FPE_OK;
}

// The poses of a host-buffer call, checked; maxRadius: the largest per-leg search radius among them.
int check_host_poses(const fpe_pose* poses, int32_t B, float& maxRadius) {
    maxRadius = 0.0f;
    for (int b = 0; b < B; ++b) {
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(poses[b].position[k]) || std::fabs(poses[b].position[k]) > 1e6)
                return fail(FPE_E_INVALID_ARG, "non-finite pose");
        if (poses[b].gait != 0 && poses[b].gait != 1) return fail(FPE_E_INVALID_ARG, "unknown gait");
        for (int l = 0; l < 4; ++l) {
            if (std::isfinite(poses[b].leg_search_radius[l])) maxRadius = std::max(maxRadius, poses[b].leg_search_radius[l]);
            if (poses[b].leg_polygon_kind[l] != 0 && poses[b].leg_polygon_kind[l] != 1)
                return fail(FPE_E_INVALID_ARG, "unknown polygon kind");
        }
    }
    return FPE_OK;
}

// The strides of a host-buffer call (null: none), checked: finite values, reserved 0.
int check_host_strides(const fpe_stride* strides, int32_t B) {
    if (!strides) return FPE_OK;
    for (int b = 0; b < B; ++b) {
        if (!std::isfinite(strides[b].step_length) || !std::isfinite(strides[b].lateral_drift))
            return fail(FPE_E_INVALID_ARG, "non-finite stride");
        if (strides[b].reserved != 0) return fail(FPE_E_INVALID_ARG, "fpe_stride.reserved must be 0");
    }
    return FPE_OK;
}

// The states of a host-buffer resume call (null: none), checked: finite values, reserved 0, 0 <= cycle and cycle + n_cycles <= 255.
int check_host_states(const fpe_plan_state* states, int32_t B, int32_t nCycles) {
    if (!states) return FPE_OK;
    for (int b = 0; b < B; ++b) {
        const double* v = &states[b].feet[0][0][0];
        for (int k = 0; k < 24; ++k)
            if (!std::isfinite(v[k])) return fail(FPE_E_INVALID_ARG, "non-finite plan state");
        if (!std::isfinite(states[b].adjusted_y)) return fail(FPE_E_INVALID_ARG, "non-finite plan state");
        if (states[b].reserved != 0) return fail(FPE_E_INVALID_ARG, "fpe_plan_state.reserved must be 0");
        if (states[b].cycle < 0 || states[b].cycle + nCycles > 255)
            return fail(FPE_E_INVALID_ARG, "fpe_plan_state.cycle must be >= 0 and cycle + n_cycles <= 255");
    }
    return FPE_OK;
}

struct GateGeom {  // what the service call's host-side (lateral) gate needs from the call's snapshot and constants
    fpe::MapGeom g;
    double isosLen, isosWid, drift;
};

// Where a host-form plan call keeps everything in its two arenas, one device and one pinned, at the same offsets, from the product
// table: [poses | strides | states | nominal | centroid | default | cycle_ok | stance | selected | status | packed | opt footholds | opt cycles
// | gate | rows | speculative flags | completion word], in 256-byte steps; the strides (fpe_plan_strides) and the states (fpe_plan_resume: state_in staged there, state_out written there, in place in a zero-copy call) next to the poses; a product that is not part of the call takes no room.
struct PlanLayout {
    size_t off[kProducts], len[kProducts];  // len 0: not in the arenas
    size_t oStrides, oStates, oSpec, oDone, total;
};
PlanLayout plan_layout(int32_t B, int32_t nCycles, const bool (&inArena)[kProducts], bool specWanted, bool stridesGiven, bool statesGiven = false) {
    PlanLayout L;
    size_t off = align256(static_cast<size_t>(B) * sizeof(fpe_pose));
    L.oStrides = off;
    off += stridesGiven ? align256(static_cast<size_t>(B) * sizeof(fpe_stride)) : 0;
    L.oStates = off;
    off += statesGiven ? align256(static_cast<size_t>(B) * sizeof(fpe_plan_state)) : 0;
    for (int k = 0; k < kProducts; ++k) {
        L.off[k] = off;
        L.len[k] = inArena[k] ? product_bytes(k, static_cast<size_t>(B), static_cast<size_t>(nCycles)) : 0;
        off += align256(L.len[k]);
    }
    // the flags of 1 the speculative chain runs on, and the chain's completion word (one-pose calls: polled by the host): plan_launches
    L.oSpec = off;
    off += specWanted ? align256(static_cast<size_t>(B) * nCycles) : 0;
    L.oDone = off;
    off += specWanted ? 256 : 0;
    L.total = off;
    return L;
}

// One host-form plan call between plan_host and its parts.
struct PlanRun {
    // set by plan_host, read by plan_launches and plan_wait_zero_copy
    int32_t B = 0, nCycles = 0;
    bool runPlan = false, runOpt = false, specWanted = false;
    // set by plan_launches: what it decided, for the wait and the copy-out
    bool zeroCopy = false, speculate = false, pollDone = false;
    uint32_t doneValue = 0;
    unsigned char* dp = nullptr;       // the arena the kernels write, as the device sees it: cx.dev, or the pinned arena itself (zeroCopy)
    const fpe_pose* dPoses = nullptr;  // where the kernels read the poses
    const fpe_stride* strides = nullptr;   // set by plan_host: the caller's strides (fpe_plan_strides), or null
    const fpe_stride* dStrides = nullptr;  // where the kernels read them
    const fpe_plan_state* stateIn = nullptr;   // set by plan_host: the caller's states (fpe_plan_resume), or null
    bool stateOutWanted = false;
    const fpe_plan_state* dStateIn = nullptr;  // where the kernels read them (the pinned arena, device-mapped) ...
    fpe_plan_state* dStateOut = nullptr;       // ... and write them (the arena the products go to, at the same offset)
    fpe_opt_out od;                    // the opt products in that arena
};

// The per-pose inputs of a host-form batch call (fpe_plan*, fpe_plan_rank*) into its pinned arena, which the kernels read
// device-mapped: the poses at its start, the strides (null: none) at oStrides behind them, the states a resume call starts from
// (null: none) at oStates behind those.
void stage_batch_inputs(unsigned char* pinned, size_t oStrides, const fpe_pose* poses, const fpe_stride* strides, int32_t B,
                        size_t oStates = 0, const fpe_plan_state* states = nullptr) {
    std::memcpy(pinned, poses, static_cast<size_t>(B) * sizeof(fpe_pose));
    if (strides) std::memcpy(pinned + oStrides, strides, static_cast<size_t>(B) * sizeof(fpe_stride));
    if (states) std::memcpy(pinned + oStates, states, static_cast<size_t>(B) * sizeof(fpe_plan_state));
}

// The launches of a host-form plan call: the plan kernel and / or the opt track's chain on cx.stream — or, speculatively, the chain
// beside the plan kernel on the side stream.
int plan_launches(fpe_engine* h, const CallPlan& cp, CallCtx& cx, const PlanLayout& L, const fpe::OptConsts& oc, const fpe_pose* poses,
                  const uint8_t* cycleOkIn, PlanRun& r) {
    unsigned char* const hp = cx.pinned;
    const int32_t B = r.B, n_cycles = r.nCycles;
    const size_t nCyc = static_cast<size_t>(B) * n_cycles;
    const size_t oOk = L.off[kCycleOk];
    stage_batch_inputs(hp, L.oStrides, poses, r.strides, B, L.oStates, r.stateIn);
    if (r.runOpt && cycleOkIn) std::memcpy(hp + oOk, cycleOkIn, nCyc);
    // Small calls (the plan_global_footholds service: one pose) skip both DMA copies: the kernels read the
    // poses from, and write their few KB of results straight into, the pinned (coherent, device-mapped) host
    // arena — two copy-engine round trips (~10 us each) less on a call whose kernel runs ~25 us.
    r.zeroCopy = L.total <= kZeroCopyBytes;
    // A small call that runs the plan AND the opt track (the service: one pose) launches the two kernels side by side: the opt
    // track's chain needs the nominal track's cycle flags only to decide whether a cycle's result is committed, and the flags are
    // all 1 unless a nominal search fails — the chain runs on a second stream on flags of 1 (L.oSpec) while the plan kernel produces
    // the real ones, and runs again, after it, in the rare call whose flags turn out otherwise (round 5: the plan kernel's ~18 us
    // off the service's latency).
    // One-pose overlapped calls (the service): the chain's last instruction writes a completion word into the pinned arena and the
    // host POLLS it (tuning key service_poll, default 1) instead of waiting for the side stream's completion signal.
    {
        std::lock_guard<std::mutex> lk(h->mu);
        r.speculate = r.specWanted && r.zeroCopy && r.runOpt && h->tuning.serviceOverlap;
        r.pollDone = r.speculate && B == 1 && h->tuning.servicePoll != 0;
    }
    // the poses are read by the kernels straight from the pinned arena (device-mapped): 64 bytes per pose, once, at the start
    // of its workgroup — a DMA transfer ahead of the launch costs its fixed fifteen microseconds before anything runs
    void* mapped = nullptr;
    FPE_HIP(hipHostGetDevicePointer(&mapped, hp, 0));
    r.dPoses = static_cast<const fpe_pose*>(mapped);
    r.dStrides = r.strides ? reinterpret_cast<const fpe_stride*>(static_cast<unsigned char*>(mapped) + L.oStrides) : nullptr;
    r.dp = r.zeroCopy ? static_cast<unsigned char*>(mapped) : cx.dev;
    unsigned char* const dp = r.dp;
    r.dStateIn = r.stateIn ? reinterpret_cast<const fpe_plan_state*>(static_cast<unsigned char*>(mapped) + L.oStates) : nullptr;
    r.dStateOut = r.stateOutWanted ? reinterpret_cast<fpe_plan_state*>(dp + L.oStates) : nullptr;
    if (!r.zeroCopy && r.runOpt && cycleOkIn) FPE_HIP(hipMemcpyAsync(dp + oOk, hp + oOk, nCyc, hipMemcpyHostToDevice, cx.stream));
    std::memset(&r.od, 0, sizeof(r.od));
    const auto queue_opt = [&]() -> int {
        if (!r.runOpt) return FPE_OK;
        for (int k = 0; k < kOptProducts; ++k) slots(r.od)[k] = L.len[kPlanProducts + k] ? dp + L.off[kPlanProducts + k] : nullptr;
        hipStream_t os = cx.stream;
        const unsigned char* okDev = dp + oOk;
        uint32_t* doneDev = nullptr;
        if (r.speculate && r.pollDone) {
            r.doneValue = ++cx.doneSeq ? cx.doneSeq : ++cx.doneSeq;  // (never 0)
            doneDev = reinterpret_cast<uint32_t*>(dp + L.oDone);
            // The counter alone says nothing about what the word holds NOW: L.oDone moves with n_cycles and the product set, and
            // the same arena takes the poses, queries and staged products of every other host-form call, and is fresh,
            // uninitialised memory after cx.reserve grew it.  Cleared here, before the chain is queued, the word can turn into
            // doneValue by the chain's own store only (nothing is in flight on this context: the last call synchronised, or its
            // chain's word was seen, before it returned).
            *reinterpret_cast<volatile uint32_t*>(hp + L.oDone) = 0;
            std::atomic_thread_fence(std::memory_order_release);
        }
        if (r.speculate) {
            std::memset(hp + L.oSpec, 1, nCyc);
            FPE_HIP(cx.side_stream(&os));
            // the chain reads both layers: the side stream waits for an asynchronous upload (fpe_upload_map_device) exactly as
            // prepare_call made cx.stream wait (the speculative chain used to start while the canonicalise / copy
            // kernels of the snapshot were still writing d_trav / d_elev)
            FPE_HIP(cp.snap->wait_ready(os));
            okDev = dp + L.oSpec;
        }
        FPE_HIP(fpe::launch_opt_track(dev_map(*cp.snap), cp.pc, oc, r.dPoses, B, n_cycles, okDev, r.od, os, doneDev, r.doneValue));
        return FPE_OK;
    };
    // (the overlapped form queues the LONGER kernel first — the chain is the call's critical path; the plan kernel's launch then costs
    // it nothing)
    if (r.speculate) {
        const int rc = queue_opt();
        if (rc != FPE_OK) return rc;
        // A polled call never enters a stream wait, and it is a stream wait (or query) that makes the runtime hand queued work to
        // the hardware at once: without it the chain was seen to END 12 us later than under hipStreamSynchronize (measured, round 6:
        // profiles/round6_service_latency.txt).  One non-blocking query per stream, right behind its launch.
        if (r.pollDone && hipStreamQuery(cx.side) != hipSuccess) (void)hipGetLastError();
    }
    if (r.runPlan) {
        fpe_plan_out d;
        for (int k = 0; k < kPlanProducts; ++k) slots(d)[k] = L.len[k] ? dp + L.off[k] : nullptr;
        // every (pose, cycle, leg) record is written by the kernel (trot: all legs each cycle; walk: each
        // leg in its phase), so the buffers need no clearing
        const int rc = launch_plan(h, cp, r.dPoses, B, n_cycles, d, cx.stream, {r.dStrides, r.dStateIn, r.dStateOut});
        if (rc != FPE_OK) return rc;
    }
    if (!r.speculate) {
        const int rc = queue_opt();
        if (rc != FPE_OK) return rc;
    }
    if (r.pollDone && hipStreamQuery(cx.stream) != hipSuccess) (void)hipGetLastError();  // (see the side stream's query above)
    return FPE_OK;
}

// The wait of a zero-copy call (the kernels wrote into the pinned arena itself): polled or synchronised, and the speculative
// chain again where the real flags differ from the ones it ran on.
int plan_wait_zero_copy(const CallPlan& cp, CallCtx& cx, const PlanLayout& L, const fpe::OptConsts& oc, const PlanRun& r) {
    unsigned char* const hp = cx.pinned;
    bool polled = false;
    if (r.pollDone && r.doneValue != 0) {
        // The chain is the call's critical path (~90 us against the plan kernel's ~20): wait for ITS word first.  Bounded: after
        // 5 ms the ordinary synchronisation below takes over (a word that never arrives must not hang the caller).
        volatile uint32_t* word = reinterpret_cast<volatile uint32_t*>(hp + L.oDone);
        const auto t0 = std::chrono::steady_clock::now();
        int spins = 0;
        while (*word != r.doneValue) {
            __builtin_ia32_pause();
            if ((++spins & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5)) break;
        }
        polled = *word == r.doneValue;
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    // (the plan kernel ended long before the chain; when the runtime has not yet seen that, wait for it the ordinary way)
    if (!(polled && hipStreamQuery(cx.stream) == hipSuccess)) {
        (void)hipGetLastError();
        FPE_HIP(hipStreamSynchronize(cx.stream));
    }
    if (r.runOpt && r.speculate) {
        // polled: every product of the chain is in the arena (its stores precede the word); the stream's own completion is
        // looked at without waiting — the context's next call queues behind it in stream order
        if (!polled) FPE_HIP(hipStreamSynchronize(cx.side));
        else if (hipStreamQuery(cx.side) != hipSuccess) (void)hipGetLastError();
        const size_t nCyc = static_cast<size_t>(r.B) * r.nCycles, oOk = L.off[kCycleOk];
        bool allCommitted = true;
        for (size_t c = 0; c < nCyc; ++c) allCommitted = allCommitted && hp[oOk + c] != 0;
        if (!allCommitted) {  // a nominal search failed in some cycle: the chain again, on the flags as they are
            FPE_HIP(fpe::launch_opt_track(dev_map(*cp.snap), cp.pc, oc, r.dPoses, r.B, r.nCycles, r.dp + oOk, r.od, cx.stream));
            FPE_HIP(hipStreamSynchronize(cx.stream));
        }
    }
    cx.inFlight = false;
    return FPE_OK;
}

// The host-buffer form of the plan and / or the opt track: one device arena (plan_layout), the launches back to back on one
// stream or side by side on two (plan_launches), the results copied out (copy_out).  `out` NULL: no plan products are returned (the
// plan still runs when the opt track needs its cycle flags and the caller gave none).
int plan_host(fpe_engine* h, const fpe_params* params, const fpe_opt_params* opt, const fpe_pose* poses, int32_t B, int32_t n_cycles,
              const fpe_plan_out* out, const uint8_t* cycleOkIn, const fpe_opt_out* oout, GateGeom* gateGeom = nullptr,
              bool* optDropped = nullptr, const fpe_stride* strides = nullptr, const fpe_plan_state* stateIn = nullptr,
              fpe_plan_state* stateOut = nullptr) {
    if (!poses || (!out && !oout)) return fail(FPE_E_INVALID_ARG, "null argument");
    if (B <= 0 || n_cycles <= 0 || n_cycles > 255) return fail(FPE_E_INVALID_ARG, "B and n_cycles must be in [1, ..] / [1, 255]");
    float maxRadius = 0.0f;
    int rcPoses = check_host_poses(poses, B, maxRadius);
    if (rcPoses != FPE_OK) return rcPoses;
    rcPoses = check_host_strides(strides, B);
    if (rcPoses != FPE_OK) return rcPoses;
    rcPoses = check_host_states(stateIn, B, n_cycles);
    if (rcPoses != FPE_OK) return rcPoses;
    if (out) {
        rcPoses = check_resumed_products(stateIn, *out);
        if (rcPoses != FPE_OK) return rcPoses;
    }
    void* want[kProducts] = {nullptr};  // the caller's arrays, by product
    if (out) std::copy(slots(*out), slots(*out) + kPlanProducts, want);
    if (oout) std::copy(slots(*oout), slots(*oout) + kOptProducts, want + kPlanProducts);
    bool inArena[kProducts];
    for (int k = 0; k < kProducts; ++k) inArena[k] = want[k] != nullptr;
    inArena[kCycleOk] = inArena[kCycleOk] || oout != nullptr;  // the opt track reads the device copy of the cycle flags
    PlanRun run;
    run.B = B;
    run.nCycles = n_cycles;
    run.runPlan = out != nullptr || (oout && !cycleOkIn);
    run.specWanted = run.runPlan && oout != nullptr && !cycleOkIn && B <= 4;
    run.strides = strides;
    run.stateIn = stateIn;
    run.stateOutWanted = stateOut != nullptr;
    const PlanLayout L = plan_layout(B, n_cycles, inArena, run.specWanted, strides != nullptr, stateIn != nullptr || stateOut != nullptr);
    if (!h) return fail(FPE_E_INVALID_ARG, "null handle or params");
    HostCall hc(h);
    CallPlan& cp = hc.cp;
    CallCtx& cx = hc.cx;
    FPE_HIP(hipSetDevice(h->device));
    FPE_HIP(cx.reserve(L.total));
    cx.inFlight = true;  // (prepare_call may already queue a bit-plane build)
    int rc = prepare_call(h, params, maxRadius, cp, cx.stream, run.runPlan);
    if (rc != FPE_OK) return rc;
    if (gateGeom) *gateGeom = GateGeom{cp.snap->g, cp.pc.isosLen, cp.pc.isosWid, cp.pc.drift};
    fpe::OptConsts oc;
    run.runOpt = oout != nullptr;
    if (oout) {
        rc = prepare_opt(params, opt, cp, maxRadius, oc);
        // optOptional: the opt track was asked for its gate verdict only (fpe_plan_service* under service_opt_gate 1 / 2) and
        // is not supported for this geometry: the plan's own products must not fail with it
        if (rc == FPE_E_UNSUPPORTED && optDropped && run.runPlan) {
            *optDropped = true;
            run.runOpt = false;
            std::fill(want + kPlanProducts, want + kProducts, nullptr);
        } else if (rc != FPE_OK) {
            return rc;
        }
    }
    rc = plan_launches(h, cp, cx, L, oc, poses, cycleOkIn, run);
    if (rc != FPE_OK) return rc;
    // ---- results to the caller ----
    SegList segs;
    segs.add(L.oStates, static_cast<size_t>(B) * sizeof(fpe_plan_state), stateOut);  // (fpe_plan_resume: the state leaves with the products)
    for (int k = 0; k < kProducts; ++k) segs.add(L.off[k], L.len[k], want[k]);
    if (!run.zeroCopy) return copy_out(h, cx, segs, run.dp, cx.pinned);
    rc = plan_wait_zero_copy(cp, cx, L, oc, run);
    if (rc != FPE_OK) return rc;
    copy_from_pinned(segs, cx.pinned);
    return FPE_OK;
}
}  // namespace

int fpe_host_alloc(fpe_handle h, size_t bytes, void** out) {
    if (!h || !out || bytes == 0) return fail(FPE_E_INVALID_ARG, "null argument");
    *out = nullptr;
    FPE_HIP(hipSetDevice(h->device));
    FPE_HIP(hipHostMalloc(out, bytes, hipHostMallocDefault));
    return FPE_OK;
}

int fpe_host_free(fpe_handle h, void* p) {
    if (!h) return fail(FPE_E_INVALID_ARG, "null handle");
    if (!p) return FPE_OK;
    FPE_HIP(hipSetDevice(h->device));
    FPE_HIP(hipHostFree(p));
    return FPE_OK;
}

int fpe_plan(fpe_handle h, const fpe_params* params, const fpe_pose* poses, int32_t B, int32_t n_cycles,
             const fpe_plan_out* out) {
    return fpe_plan_strides(h, params, poses, nullptr, B, n_cycles, out);
}

int fpe_plan_strides(fpe_handle h, const fpe_params* params, const fpe_pose* poses, const fpe_stride* strides, int32_t B, int32_t n_cycles,
                     const fpe_plan_out* out) {
    return fpe_plan_resume(h, params, poses, strides, nullptr, B, n_cycles, out, nullptr);
}

int fpe_plan_resume(fpe_handle h, const fpe_params* params, const fpe_pose* poses, const fpe_stride* strides, const fpe_plan_state* state_in,
                    int32_t B, int32_t n_cycles, const fpe_plan_out* out, fpe_plan_state* state_out) {
    if (!out) return fail(FPE_E_INVALID_ARG, "null argument");
    return plan_host(h, params, nullptr, poses, B, n_cycles, out, nullptr, nullptr, nullptr, nullptr, strides, state_in, state_out);
}

int fpe_plan_opt(fpe_handle h, const fpe_params* params, const fpe_opt_params* opt, const fpe_pose* poses, int32_t B,
                 int32_t n_cycles, const uint8_t* cycle_ok, const fpe_opt_out* out) {
    if (!out) return fail(FPE_E_INVALID_ARG, "null argument");
    return plan_host(h, params, opt, poses, B, n_cycles, nullptr, cycle_ok, out);
}

int fpe_plan_opt_device(fpe_handle h, const fpe_params* params, const fpe_opt_params* opt, const fpe_pose* d_poses, int32_t B,
                        int32_t n_cycles, const uint8_t* d_cycle_ok, const fpe_opt_out* d_out, void* stream) {
    if (!d_poses || !d_out || !d_cycle_ok) return fail(FPE_E_INVALID_ARG, "null argument");
    if (B <= 0 || n_cycles <= 0 || n_cycles > 255) return fail(FPE_E_INVALID_ARG, "B and n_cycles must be in [1, ..] / [1, 255]");
    hipStream_t st = static_cast<hipStream_t>(stream);
    CallPlan cp;
    int rc = prepare_call(h, params, 0.0f, cp, st, false);
    if (rc != FPE_OK) return rc;
    fpe::OptConsts oc;
    rc = prepare_opt(params, opt, cp, std::max(params->searchRadius, cp.pc.maxSearchRadius), oc);
    if (rc != FPE_OK) return rc;
    mark_async_launch(cp);
    FPE_HIP(fpe::launch_opt_track(dev_map(*cp.snap), cp.pc, oc, d_poses, B, n_cycles, d_cycle_ok, *d_out, st));
    return FPE_OK;
}

int fpe_search_legs_device(fpe_handle h, const fpe_params* params, const fpe_leg_query* d_queries, int32_t n,
                           fpe_foothold* d_out, void* stream) {
    if (!d_queries || !d_out) return fail(FPE_E_INVALID_ARG, "null argument");
    if (n <= 0) return fail(FPE_E_INVALID_ARG, "n must be positive");
    hipStream_t st = static_cast<hipStream_t>(stream);
    CallPlan cp;
    int rc = prepare_call(h, params, 0.0f, cp, st, false);
    if (rc != FPE_OK) return rc;
    mark_async_launch(cp);
    FPE_HIP(fpe::launch_search_legs(dev_map(*cp.snap), cp.pc, h->lut(), d_queries, n, d_out, st));
    return FPE_OK;
}

int fpe_search_legs(fpe_handle h, const fpe_params* params, const fpe_leg_query* queries, int32_t n, fpe_foothold* out) {
    if (!queries || !out) return fail(FPE_E_INVALID_ARG, "null argument");
    if (n <= 0) return fail(FPE_E_INVALID_ARG, "n must be positive");
    float maxRadius = 0.0f;
    for (int k = 0; k < n; ++k) {
        if (!std::isfinite(queries[k].cx) || !std::isfinite(queries[k].cy) || std::fabs(queries[k].cx) > 1e6 ||
            std::fabs(queries[k].cy) > 1e6)
            return fail(FPE_E_INVALID_ARG, "non-finite query centre");
        if (!(queries[k].search_radius >= 0.0f) || !std::isfinite(queries[k].search_radius))
            return fail(FPE_E_INVALID_ARG, "bad search radius");
        if (queries[k].n_vertices < 0 || queries[k].n_vertices > FPE_MAX_POLYGON_VERTICES)
            return fail(FPE_E_INVALID_ARG, "too many polygon vertices");
        maxRadius = std::max(maxRadius, queries[k].search_radius);
    }
    return query_round_trip(h, params, maxRadius, queries, n, out,
                            [&](const CallPlan& cp, const fpe_leg_query* d_q, fpe_foothold* d_out, hipStream_t s) {
                                return fpe::launch_search_legs(dev_map(*cp.snap), cp.pc, h->lut(), d_q, n, d_out, s);
                            });
}

int fpe_foothold_map_device(fpe_handle h, const fpe_params* params, const int32_t roi[4], const fpe_foothold_map_out* d_out,
                            void* stream) {
    if (!d_out) return fail(FPE_E_INVALID_ARG, "null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    CallPlan cp;
    fpe::FootmapRoi r{};
    int rc = prepare_foothold_map(h, params, roi, d_out->flags || d_out->height, cp, r, st);
    if (rc != FPE_OK) return rc;
    mark_async_launch(cp);
    FPE_HIP(fpe::launch_foothold_map(dev_map(*cp.snap), cp.bits, cp.pc, r, d_out->flags, d_out->height, st));
    return FPE_OK;
}

int fpe_foothold_map(fpe_handle h, const fpe_params* params, const int32_t roi[4], const fpe_foothold_map_out* out) {
    if (!out) return fail(FPE_E_INVALID_ARG, "null argument");
    if (!h) return fail(FPE_E_INVALID_ARG, "null handle or params");
    HostCall hc(h);
    CallPlan& cp = hc.cp;
    CallCtx& cx = hc.cx;
    FPE_HIP(hipSetDevice(h->device));
    FPE_HIP(cx.reserve(0));  // the stream
    fpe::FootmapRoi r{};
    int rc = prepare_foothold_map(h, params, roi, out->flags || out->height, cp, r, cx.stream);
    if (rc != FPE_OK) return rc;
    const size_t n = static_cast<size_t>(r.nr) * r.nc;
    const HostProduct prod[2] = {{out->flags, n}, {out->height, n * sizeof(float)}};
    return stage_products(cx, prod, [&](unsigned char* const* d, hipStream_t s) {
        return fpe::launch_foothold_map(dev_map(*cp.snap), cp.bits, cp.pc, r, d[0], reinterpret_cast<float*>(d[1]), s);
    });
}

int fpe_foothold_snap_device(fpe_handle h, const fpe_params* params, const int32_t roi[4], float search_radius, int32_t polygon_kind,
                             const fpe_foothold_snap_out* d_out, void* stream) {
    if (!d_out) return fail(FPE_E_INVALID_ARG, "null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    CallPlan cp;
    fpe::FootmapRoi r{};
    fpe::SnapConsts sc{};
    bool bitPath = false;
    int rc = prepare_foothold_snap(h, params, roi, search_radius, polygon_kind, d_out->offset || d_out->source || d_out->z, d_out->z != nullptr,
                                   cp, r, sc, bitPath, st);
    if (rc != FPE_OK) return rc;
    mark_async_launch(cp);
    FPE_HIP(run_foothold_snap(h, cp, r, sc, bitPath, d_out->offset, d_out->source, d_out->z, st));
    return FPE_OK;
}

int fpe_foothold_snap(fpe_handle h, const fpe_params* params, const int32_t roi[4], float search_radius, int32_t polygon_kind,
                      const fpe_foothold_snap_out* out) {
    if (!out) return fail(FPE_E_INVALID_ARG, "null argument");
    if (!h) return fail(FPE_E_INVALID_ARG, "null handle or params");
    HostCall hc(h);
    CallPlan& cp = hc.cp;
    CallCtx& cx = hc.cx;
    FPE_HIP(hipSetDevice(h->device));
    FPE_HIP(cx.reserve(0));  // the stream
    fpe::FootmapRoi r{};
    fpe::SnapConsts sc{};
    bool bitPath = false;
    int rc = prepare_foothold_snap(h, params, roi, search_radius, polygon_kind, out->offset || out->source || out->z, out->z != nullptr,
                                   cp, r, sc, bitPath, cx.stream);
    if (rc != FPE_OK) return rc;
    const size_t n = static_cast<size_t>(r.nr) * r.nc;
    const HostProduct prod[3] = {{out->offset, 2 * n}, {out->source, n}, {out->z, n * sizeof(float)}};
    return stage_products(cx, prod, [&](unsigned char* const* d, hipStream_t s) {
        return run_foothold_snap(h, cp, r, sc, bitPath, reinterpret_cast<int8_t*>(d[0]), d[1], reinterpret_cast<float*>(d[2]), s);
    });
}

int fpe_centroid_legs_device(fpe_handle h, const fpe_params* params, const fpe_centroid_query* d_queries, int32_t n,
                             fpe_centroid_foothold* d_out, void* stream) {
    if (!d_queries || !d_out) return fail(FPE_E_INVALID_ARG, "null argument");
    if (n <= 0) return fail(FPE_E_INVALID_ARG, "n must be positive");
    hipStream_t st = static_cast<hipStream_t>(stream);
    CallPlan cp;
    int rc = prepare_call(h, params, 0.0f, cp, st, false);
    if (rc != FPE_OK) return rc;
    mark_async_launch(cp);
    FPE_HIP(fpe::launch_centroid_legs(dev_map(*cp.snap), cp.pc, params->searchRadius, d_queries, n, d_out, st));
    return FPE_OK;
}

int fpe_centroid_legs(fpe_handle h, const fpe_params* params, const fpe_centroid_query* queries, int32_t n, fpe_centroid_foothold* out) {
    if (!queries || !out) return fail(FPE_E_INVALID_ARG, "null argument");
    if (n <= 0) return fail(FPE_E_INVALID_ARG, "n must be positive");
    for (int k = 0; k < n; ++k)  // any centre is a query (code 6 off the map); a radius must be a number
        if (!std::isfinite(queries[k].search_radius)) return fail(FPE_E_INVALID_ARG, "bad search radius");
    return query_round_trip(h, params, 0.0f, queries, n, out,
                            [&](const CallPlan& cp, const fpe_centroid_query* d_q, fpe_centroid_foothold* d_out, hipStream_t s) {
                                return fpe::launch_centroid_legs(dev_map(*cp.snap), cp.pc, params->searchRadius, d_q, n, d_out, s);
                            });
}

int fpe_centroid_map_device(fpe_handle h, const fpe_params* params, const int32_t roi[4], float search_radius,
                            const fpe_centroid_map_out* d_out, void* stream) {
    if (!d_out) return fail(FPE_E_INVALID_ARG, "null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    CallPlan cp;
    fpe::FootmapRoi r{};
    fpe::CmapConsts cc{};
    int rc = prepare_centroid_map(h, params, roi, search_radius, d_out->code || d_out->offset || d_out->z, cp, r, cc, st);
    if (rc != FPE_OK) return rc;
    mark_async_launch(cp);
    FPE_HIP(run_centroid_map(cp, r, cc, d_out->code, d_out->offset, d_out->z, st));
    return FPE_OK;
}

int fpe_centroid_map(fpe_handle h, const fpe_params* params, const int32_t roi[4], float search_radius, const fpe_centroid_map_out* out) {
    if (!out) return fail(FPE_E_INVALID_ARG, "null argument");
    if (!h) return fail(FPE_E_INVALID_ARG, "null handle or params");
    HostCall hc(h);
    CallPlan& cp = hc.cp;
    CallCtx& cx = hc.cx;
    FPE_HIP(hipSetDevice(h->device));
    FPE_HIP(cx.reserve(0));  // the stream
    fpe::FootmapRoi r{};
    fpe::CmapConsts cc{};
    int rc = prepare_centroid_map(h, params, roi, search_radius, out->code || out->offset || out->z, cp, r, cc, cx.stream);
    if (rc != FPE_OK) return rc;
    const size_t n = static_cast<size_t>(r.nr) * r.nc;
    const HostProduct prod[3] = {{out->code, n}, {out->offset, 2 * n}, {out->z, n * sizeof(float)}};
    return stage_products(cx, prod, [&](unsigned char* const* d, hipStream_t s) {
        return run_centroid_map(cp, r, cc, d[0], reinterpret_cast<int8_t*>(d[1]), reinterpret_cast<float*>(d[2]), s);
    });
}

int fpe_export_layers_device(fpe_handle h, const fpe_params* params, const int32_t roi[4], const fpe_layer_layout* layout,
                             const fpe_layer_request* d_request, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    ExportPlan xp;
    const int rc = prepare_export_layers(h, params, roi, layout, d_request, xp, st);
    // (also behind a refusal that follows a family's prepare: that prepare may have queued the planes' build on `stream`)
    for (int f = 0; f < kExportFamilies; ++f)
        if (xp.prepared[f]) mark_async_launch(xp.cp[f]);
    if (rc != FPE_OK) return rc;
    FPE_HIP(run_export_layers(h, xp, *d_request, d_request->dst, st));
    return FPE_OK;
}

int fpe_export_layers(fpe_handle h, const fpe_params* params, const int32_t roi[4], const fpe_layer_layout* layout,
                      const fpe_layer_request* request) {
    if (!h) return fail(FPE_E_INVALID_ARG, "null handle, params or request");
    ExportPlan xp;  // ahead of the lease: the stream is waited for before the snapshot and the planes are released (HostCall)
    HostCall hc(h);
    CallCtx& cx = hc.cx;
    FPE_HIP(hipSetDevice(h->device));
    FPE_HIP(cx.reserve(0));  // the stream
    const int rc = prepare_export_layers(h, params, roi, layout, request, xp, cx.stream);
    if (rc != FPE_OK) return rc;
    const size_t bytes = static_cast<size_t>(xp.args.rows) * xp.args.cols * sizeof(float);
    HostProduct prod[FPE_LAYER_COUNT] = {};
    for (int k = 0; k < request->n_layers; ++k) prod[k] = HostProduct{request->dst[k], bytes};
    return stage_products(cx, prod, [&](unsigned char* const* d, hipStream_t s) {
        float* d_dst[FPE_LAYER_COUNT];
        for (int k = 0; k < FPE_LAYER_COUNT; ++k) d_dst[k] = reinterpret_cast<float*>(d[k]);
        return run_export_layers(h, xp, *request, d_dst, s);
    });
}

int fpe_rank_params_defaults(fpe_rank_params* out) {
    if (!out) return fail(FPE_E_INVALID_ARG, "null argument");
    std::memset(out, 0, sizeof(*out));
    out->w_fail = 100.0;
    out->w_spiral = 1.0;
    out->w_none = 0.0;
    out->w_deviation = 10.0;
    out->w_speed_spread = 0.0;
    out->min_cycles = 0;
    return FPE_OK;
}

namespace {
// Arguments of fpe_plan_rank* that need no map; rc: the ranking's constants (rank NULL: the defaults).
int check_rank_args(const fpe_params* params, const fpe_rank_params* rank, int32_t B, int32_t n_cycles, int32_t K, const fpe_rank_out* out,
                    fpe::RankConsts& rc) {
    if (!params || !out || !out->best) return fail(FPE_E_INVALID_ARG, "null argument");
    if (B <= 0 || n_cycles <= 0 || n_cycles > 255) return fail(FPE_E_INVALID_ARG, "B and n_cycles must be in [1, ..] / [1, 255]");
    if (K < 1 || K > B || K > 1024) return fail(FPE_E_INVALID_ARG, "K must be in [1, min(B, 1024)]");
    fpe_rank_params def;
    if (!rank) {
        fpe_rank_params_defaults(&def);
        rank = &def;
    }
    const double w[5] = {rank->w_fail, rank->w_spiral, rank->w_none, rank->w_deviation, rank->w_speed_spread};
    for (double v : w)
        if (!std::isfinite(v)) return fail(FPE_E_INVALID_ARG, "rank weights must be finite");
    if (rank->min_cycles < 0 || rank->min_cycles > 255) return fail(FPE_E_INVALID_ARG, "min_cycles must be in [0, 255]");
    rc = fpe::RankConsts{w[0], w[1], w[2], w[3], w[4], static_cast<double>(params->stepLength / 2), rank->min_cycles, params->RF_FIRST};
    return FPE_OK;
}

// What the host forms of the ranking and beam calls open with, on the lease `hc` of the caller: the arenas, the prepare, the two
// refusals that need the map, and the pinned arena as the device sees it (`mapped`: the kernels read the call's inputs there, as in
// fpe_plan; the caller stages them).
int open_batch_call(fpe_engine* h, HostCall& hc, const fpe_params* params, float maxRadius, size_t arenaBytes, bool packedWanted,
                    fpe::PlanForm form, unsigned char*& mapped) {
    CallCtx& cx = hc.cx;
    FPE_HIP(hipSetDevice(h->device));
    FPE_HIP(cx.reserve(arenaBytes));
    cx.inFlight = true;  // (prepare_call may already queue a bit-plane build)
    int rc = prepare_call(h, params, maxRadius, hc.cp, cx.stream, true);
    if (rc != FPE_OK) return rc;
    rc = check_packed_fits(hc.cp, packedWanted);
    if (rc != FPE_OK) return rc;
    rc = check_strides_launchable(hc.cp, form);
    if (rc != FPE_OK) return rc;
    void* p = nullptr;
    FPE_HIP(hipHostGetDevicePointer(&p, cx.pinned, 0));
    mapped = static_cast<unsigned char*>(p);
    return FPE_OK;
}

// Where everything a ranking call touches on the device lives.  `full`: the un-compacted products — the caller's (d_full) where given,
// scratch for what the ranking reads or the compaction copies from, null for the rest.  The B-sized and K-sized outputs are the
// caller's own arrays (the device form) or — the host form — lie in the output block in the order products, summary, score, best,
// n_class0; summary and score go to scratch when the caller did not ask for them.
struct RankLayout {
    int32_t B, n, K;
    fpe_plan_out full, best;
    fpe_pose_summary* summary;
    double* score;
    int32_t* bestIdx;
    int32_t* nClass0;
    void* keys;
};
static_assert(kPlanProducts + 4 + 5 <= kMaxSegs, "SegList holds a (checked) ranking call's outputs");
void rank_layout(RankLayout& L, ArenaCursor& A, const fpe_plan_out* dFull, const fpe_rank_out& want, bool hostForm) {
    const bool reads[kPlanProducts] = {true, false, true, true, true, false, true, false};  // rank_summary_kernel's inputs
    const size_t B = static_cast<size_t>(L.B), K = static_cast<size_t>(L.K), n = static_cast<size_t>(L.n);
    const auto out = [&](void* dst, size_t bytes) { return (dst && hostForm) ? A.out(dst, bytes) : dst; };
    void* const* given = dFull ? slots(*dFull) : nullptr;
    void* const* wanted = slots(want.best_products);
    for (int k = 0; k < kPlanProducts; ++k) {
        slots(L.full)[k] = (given && given[k]) ? given[k] : ((reads[k] || wanted[k]) ? A.take(product_bytes(k, B, n)) : nullptr);
        slots(L.best)[k] = out(wanted[k], product_bytes(k, K, n));
    }
    const size_t szSum = B * sizeof(fpe_pose_summary), szScore = B * sizeof(double);
    L.summary = static_cast<fpe_pose_summary*>(want.summary ? out(want.summary, szSum) : A.take(szSum));
    L.score = static_cast<double*>(want.score ? out(want.score, szScore) : A.take(szScore));
    L.bestIdx = static_cast<int32_t*>(out(want.best, K * sizeof(int32_t)));
    L.nClass0 = static_cast<int32_t*>(out(want.n_class0, sizeof(int32_t)));
    L.keys = A.take(fpe::rank_scratch_bytes(L.B, L.K));
}

// The launches of a prepared ranking call on `stream`: the plan through launch_plan, then summary, (check: the check stage of a
// checked ranking,) select, gather.
int run_rank(fpe_engine* h, const CallPlan& cp, const fpe::RankConsts& rc, const fpe_pose* d_poses, const fpe_stride* d_strides, const RankLayout& L,
             hipStream_t stream, const fpe::CheckStage* check) {
    int rc0 = launch_plan(h, cp, d_poses, L.B, L.n, L.full, stream, {d_strides});
    if (rc0 != FPE_OK) return rc0;
    FPE_HIP(fpe::launch_rank(rc, d_poses, L.B, L.n, L.K, L.full, L.summary, L.score, L.keys, L.bestIdx, L.nClass0, L.best, stream, d_strides,
                             check));
    return FPE_OK;
}

// The check stage of a checked ranking (fpe_plan_rank_checked*; defined with them, behind the three checks' host functions).  Both
// ranking forms take one — null: a plain ranking, every step below skipped — and call, in this order:
struct CheckCall;
int check_call_map(CheckCall& cc, const CallPlan& cp);  // the refusals that need the snapshot; the margin's constants
// the check outputs behind the ranking's in the layout (the host form: in the output block)
void check_call_layout(CheckCall& cc, ArenaCursor& A, int32_t B, bool hostForm);
int check_call_planes(CheckCall& cc, const fpe_params& params, const CallPlan& cp, hipStream_t stream);  // the margin's bit planes
void check_call_mark_async(const CheckCall& cc);
// what launch_rank takes: the stage on the layout's products; null when there is nothing to launch
const fpe::CheckStage* check_call_stage(CheckCall& cc, const CallPlan& cp, const RankLayout& L);

int rank_device_call(fpe_handle h, const fpe_params* params, const fpe_rank_params* rank, CheckCall* check, const fpe_pose* d_poses,
                     const fpe_stride* d_strides, int32_t B, int32_t n_cycles, int32_t K, const fpe_plan_out* d_full, const fpe_rank_out* d_out,
                     void* stream);
int rank_host_call(fpe_handle h, const fpe_params* params, const fpe_rank_params* rank, CheckCall* check, const fpe_pose* poses,
                   const fpe_stride* strides, int32_t B, int32_t n_cycles, int32_t K, const fpe_rank_out* out);
}  // namespace

int fpe_plan_rank_device(fpe_handle h, const fpe_params* params, const fpe_rank_params* rank, const fpe_pose* d_poses, int32_t B,
                         int32_t n_cycles, int32_t K, const fpe_plan_out* d_full, const fpe_rank_out* d_out, void* stream) {
    return fpe_plan_rank_strides_device(h, params, rank, d_poses, nullptr, B, n_cycles, K, d_full, d_out, stream);
}

int fpe_plan_rank_strides_device(fpe_handle h, const fpe_params* params, const fpe_rank_params* rank, const fpe_pose* d_poses,
                                 const fpe_stride* d_strides, int32_t B, int32_t n_cycles, int32_t K, const fpe_plan_out* d_full,
                                 const fpe_rank_out* d_out, void* stream) {
    return rank_device_call(h, params, rank, nullptr, d_poses, d_strides, B, n_cycles, K, d_full, d_out, stream);
}

namespace {
// The device form of every ranking call; rank's and check's arguments that need no map are checked by the caller's entry point
// (check) and here (rank).
int rank_device_call(fpe_handle h, const fpe_params* params, const fpe_rank_params* rank, CheckCall* check, const fpe_pose* d_poses,
                     const fpe_stride* d_strides, int32_t B, int32_t n_cycles, int32_t K, const fpe_plan_out* d_full, const fpe_rank_out* d_out,
                     void* stream) {
    fpe::RankConsts rc;
    int rc0 = check_rank_args(params, rank, B, n_cycles, K, d_out, rc);
    if (rc0 != FPE_OK) return rc0;
    if (!d_poses) return fail(FPE_E_INVALID_ARG, "null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    CallPlan cp;
    rc0 = prepare_call(h, params, 0.0f, cp, st, true);
    if (rc0 != FPE_OK) return rc0;
    RankLayout L{};
    L.B = B, L.n = n_cycles, L.K = K;
    ArenaCursor sizes;
    rank_layout(L, sizes, d_full, *d_out, false);
    rc0 = check_packed_fits(cp, (d_full && d_full->selected_packed) || d_out->best_products.selected_packed);
    if (rc0 != FPE_OK) return rc0;
    rc0 = check_strides_launchable(cp, d_strides ? fpe::PlanForm::Stride : fpe::PlanForm::Plain);
    if (rc0 != FPE_OK) return rc0;
    if (check) {
        rc0 = check_call_map(*check, cp);
        if (rc0 == FPE_OK) rc0 = check_call_planes(*check, *params, cp, st);
        if (rc0 != FPE_OK) return rc0;
        check_call_mark_async(*check);
    }
    mark_async_launch(cp);
    return with_stream_scratch(sizes.scratchBytes, st, [&](unsigned char* scratch) {
        ArenaCursor A{scratch};
        rank_layout(L, A, d_full, *d_out, false);
        if (check) check_call_layout(*check, A, B, false);
        return run_rank(h, cp, rc, d_poses, d_strides, L, st, check ? check_call_stage(*check, cp, L) : nullptr);
    });
}
}  // namespace

int fpe_plan_rank(fpe_handle h, const fpe_params* params, const fpe_rank_params* rank, const fpe_pose* poses, int32_t B, int32_t n_cycles,
                  int32_t K, const fpe_rank_out* out) {
    return fpe_plan_rank_strides(h, params, rank, poses, nullptr, B, n_cycles, K, out);
}

int fpe_plan_rank_strides(fpe_handle h, const fpe_params* params, const fpe_rank_params* rank, const fpe_pose* poses, const fpe_stride* strides,
                          int32_t B, int32_t n_cycles, int32_t K, const fpe_rank_out* out) {
    return rank_host_call(h, params, rank, nullptr, poses, strides, B, n_cycles, K, out);
}

namespace {
// The host form of every ranking call (as rank_device_call)
int rank_host_call(fpe_handle h, const fpe_params* params, const fpe_rank_params* rank, CheckCall* check, const fpe_pose* poses,
                   const fpe_stride* strides, int32_t B, int32_t n_cycles, int32_t K, const fpe_rank_out* out) {
    fpe::RankConsts rc;
    int rc0 = check_rank_args(params, rank, B, n_cycles, K, out, rc);
    if (rc0 != FPE_OK) return rc0;
    if (!h || !poses) return fail(FPE_E_INVALID_ARG, "null argument");
    float maxRadius = 0.0f;
    rc0 = check_host_poses(poses, B, maxRadius);
    if (rc0 != FPE_OK) return rc0;
    rc0 = check_host_strides(strides, B);
    if (rc0 != FPE_OK) return rc0;
    RankLayout L{};
    L.B = B, L.n = n_cycles, L.K = K;
    ArenaCursor sizes;
    rank_layout(L, sizes, nullptr, *out, true);
    if (check) check_call_layout(*check, sizes, B, true);
    // both arenas: [poses (| strides) | outputs | scratch].  The poses are read from the pinned arena (device-mapped), as in fpe_plan; outputs of up
    // to kZeroCopyBytes are WRITTEN there by the kernels too (no transfer at all: a DMA costs some ten microseconds, whatever its size)
    const size_t oStrides = align256(static_cast<size_t>(B) * sizeof(fpe_pose));
    const size_t szPose = oStrides + (strides ? align256(static_cast<size_t>(B) * sizeof(fpe_stride)) : 0);  // (the per-pose inputs)
    const bool zeroCopy = sizes.outBytes <= kZeroCopyBytes;
    HostCall hc(h);
    CallCtx& cx = hc.cx;
    unsigned char* mapped = nullptr;
    rc0 = open_batch_call(h, hc, params, maxRadius, szPose + sizes.outBytes + sizes.scratchBytes, out->best_products.selected_packed != nullptr,
                          strides ? fpe::PlanForm::Stride : fpe::PlanForm::Plain, mapped);
    if (rc0 != FPE_OK) return rc0;
    if (check) {
        rc0 = check_call_map(*check, hc.cp);
        if (rc0 == FPE_OK) rc0 = check_call_planes(*check, *params, hc.cp, cx.stream);
        if (rc0 != FPE_OK) return rc0;
    }
    stage_batch_inputs(cx.pinned, oStrides, poses, strides, B);
    ArenaCursor A{cx.dev + szPose + sizes.outBytes, (zeroCopy ? mapped : cx.dev) + szPose, szPose};
    rank_layout(L, A, nullptr, *out, true);
    if (check) check_call_layout(*check, A, B, true);
    const fpe_stride* dStrides = strides ? reinterpret_cast<const fpe_stride*>(mapped + oStrides) : nullptr;
    rc0 = run_rank(h, hc.cp, rc, reinterpret_cast<const fpe_pose*>(mapped), dStrides, L, cx.stream,
                   check ? check_call_stage(*check, hc.cp, L) : nullptr);
    if (rc0 != FPE_OK) return rc0;
    if (!zeroCopy) return copy_out(h, cx, A.outs, cx.dev, cx.pinned);
    FPE_HIP(hipStreamSynchronize(cx.stream));
    cx.inFlight = false;
    copy_from_pinned(A.outs, cx.pinned);
    return FPE_OK;
}
}  // namespace

int fpe_beam_params_defaults(fpe_beam_params* out) {
    if (!out) return fail(FPE_E_INVALID_ARG, "null argument");
    std::memset(out, 0, sizeof(*out));
    out->segments = 4;
    out->cycles_per_segment = 2;
    out->width = 8;
    out->w_fail = 100.0;
    out->w_spiral = 1.0;
    out->w_none = 0.0;
    out->w_deviation = 10.0;
    out->w_progress = 100.0;
    return FPE_OK;
}

namespace {
constexpr int kBeamOwn = 5;  // a beam call's outputs of its own, behind the products: n_live, score, penalty, path, state
constexpr int kBeamCheckOwn = 6;  // a checked beam's, behind those: the three summaries, base_penalty, hit, feet
static_assert(kPlanProducts + kBeamOwn + kBeamCheckOwn <= kMaxSegs, "SegList holds a (checked) beam call's outputs");

// Arguments of fpe_plan_beam* that need no map; bc / sh: the beam's constants and shape (beam NULL: the defaults).
int check_beam_args(const fpe_params* params, const fpe_beam_params* beam, int32_t B, int32_t M, const fpe_beam_out* out, fpe::BeamConsts& bc,
                    fpe::BeamShape& sh) {
    if (!params || !out || !out->path) return fail(FPE_E_INVALID_ARG, "null argument (path is required)");
    fpe_beam_params def;
    if (!beam) {
        fpe_beam_params_defaults(&def);
        beam = &def;
    }
    const int32_t S = beam->segments, k = beam->cycles_per_segment, W = beam->width;
    if (B < 1 || M < 1 || M > FPE_BEAM_MAX_OPTIONS || W < 1 || W > FPE_BEAM_MAX_WIDTH)
        return fail(FPE_E_INVALID_ARG, "beam: B >= 1, 1 <= M <= 16 and 1 <= width <= 64");
    if (S < 1 || k < 1 || static_cast<long long>(S) * k > 255) return fail(FPE_E_INVALID_ARG, "beam: segments, cycles_per_segment >= 1 and their product <= 255");
    if (static_cast<long long>(B) * W * M > FPE_BEAM_MAX_CHAINS) return fail(FPE_E_INVALID_ARG, "beam: B * width * M exceeds FPE_BEAM_MAX_CHAINS");
    if (beam->reserved != 0) return fail(FPE_E_INVALID_ARG, "fpe_beam_params.reserved must be 0");
    const double w[5] = {beam->w_fail, beam->w_spiral, beam->w_none, beam->w_deviation, beam->w_progress};
    for (double v : w)
        if (!std::isfinite(v)) return fail(FPE_E_INVALID_ARG, "beam weights must be finite");
    if (out->products.stance || out->products.pose_status)
        return fail(FPE_E_INVALID_ARG, "a beam's plans are continuations: no stance and no pose_status");
    bc = fpe::BeamConsts{w[0], w[1], w[2], w[3], w[4]};
    sh = fpe::BeamShape{B, M, W, S, k, 0, W};
    sh.slotStride = fpe::beam_live(sh, S - 1);
    return FPE_OK;
}

// Where everything a beam call touches on the device lives: the scratch (fpe::BeamScratch) and — the host form — the output block,
// dense (outStride = n_{S-1} slots per root), in the order products, n_live, score, penalty, path, state.  outSlot[q]: bytes per
// slot of transfer q of the cursor's list (0: one element per root), for the underfilled repack.
struct BeamLayout {
    fpe::BeamShape sh;
    fpe::BeamScratch sc;
    fpe_beam_out out;
    size_t outSlot[kPlanProducts + kBeamOwn + kBeamCheckOwn];
};
// The check stage of a checked beam (fpe_plan_beam_checked*; defined with them, behind the checked ranking).  Both beam forms take
// one — null: a plain beam, every step below skipped, the launches those of fpe_plan_beam* — and call, in this order:
struct BeamCheckCall;
// the refusals that need the snapshot; the margin's constants; the lane mapping of the check kernel
int beam_check_map(fpe_engine* h, BeamCheckCall& bc, const fpe_params& params, const CallPlan& cp);
// the candidates' and parents' check states in the scratch, the check outputs behind the beam's in the layout
void beam_check_layout(BeamCheckCall& bc, BeamLayout& L, ArenaCursor& A, bool hostForm);
int beam_check_planes(BeamCheckCall& bc, const fpe_params& params, const CallPlan& cp, hipStream_t stream);  // the margin's bit planes
void beam_check_mark_async(const BeamCheckCall& bc);
bool beam_check_wants_stance(const BeamCheckCall& bc, bool haveStateIn);  // segment 0's plan writes the roots' start feet
// score / select / keep of segment s and the trace with the checks folded in (launch_beam_prune's and launch_beam_trace's places)
int beam_check_prune(BeamCheckCall& bc, const CallPlan& cp, const fpe::BeamConsts& consts, const BeamLayout& L, int s, hipStream_t stream);
int beam_check_trace(BeamCheckCall& bc, const BeamLayout& L, hipStream_t stream);

void beam_layout(BeamLayout& L, ArenaCursor& A, const fpe_beam_out& want, bool hostForm, bool wantStance = false) {
    // beam_score_kernel's inputs (wantStance: a checked beam from the poses, whose roots start from the stance)
    const bool reads[kPlanProducts] = {true, false, true, true, wantStance, false, false, false};
    const fpe::BeamShape& sh = L.sh;
    const size_t S = static_cast<size_t>(sh.S), k = static_cast<size_t>(sh.k), slots_ = static_cast<size_t>(sh.B) * sh.slotStride;
    const size_t chains = static_cast<size_t>(sh.B) * (sh.S > 1 ? fpe::beam_live(sh, sh.S - 2) : 1) * sh.M;
    const size_t outSlots = static_cast<size_t>(sh.B) * sh.outStride;
    const auto out = [&](void* dst, size_t bytesPerSlot, bool perRoot = false) {
        if (!dst || !hostForm) return dst;
        L.outSlot[A.outs.n] = perRoot ? 0 : bytesPerSlot;
        return A.out(dst, bytesPerSlot * (perRoot ? static_cast<size_t>(sh.B) : outSlots));
    };
    L.sc.poses = A.take_n<fpe_pose>(chains);
    L.sc.strides = A.take_n<fpe_stride>(chains);
    L.sc.stateIn = A.take_n<fpe_plan_state>(chains);
    L.sc.stateOut = A.take_n<fpe_plan_state>(chains);
    L.sc.candPenalty = A.take_n<double>(chains);
    L.sc.candScore = A.take_n<double>(chains);
    L.sc.keys = A.take(chains * 16);
    L.sc.surv = A.take_n<fpe::BeamSurvivor>(S * slots_);
    L.sc.parents = A.take_n<fpe_plan_state>(slots_);
    void* const* wanted = slots(want.products);
    for (int q = 0; q < kPlanProducts; ++q) {
        slots(L.sc.cand)[q] = (reads[q] || wanted[q]) ? A.take(product_bytes(q, chains, k)) : nullptr;
        slots(L.sc.hist)[q] = wanted[q] ? A.take(product_bytes(q, S * slots_, k)) : nullptr;
        slots(L.out.products)[q] = out(wanted[q], product_bytes(q, 1, S * k));
    }
    L.out.n_live = static_cast<int32_t*>(out(want.n_live, sizeof(int32_t), true));
    L.out.score = static_cast<double*>(out(want.score, sizeof(double)));
    L.out.penalty = static_cast<double*>(out(want.penalty, sizeof(double)));
    L.out.path = static_cast<uint8_t*>(out(want.path, S));
    L.out.state = static_cast<fpe_plan_state*>(out(want.state, sizeof(fpe_plan_state)));
}

// The launches of a prepared beam call on `stream`: S x (expand, the resume kernels through launch_plan, score / select / keep),
// then the trace.  Nothing synchronises the host.
int run_beam(fpe_engine* h, const CallPlan& cp, const fpe::BeamConsts& bc, const fpe_pose* d_poses, const fpe_stride* d_options,
             const fpe_plan_state* d_stateIn, const BeamLayout& L, hipStream_t stream, BeamCheckCall* check) {
    const fpe::BeamShape& sh = L.sh;
    for (int s = 0; s < sh.S; ++s) {
        FPE_HIP(fpe::launch_beam_expand(sh, s, d_poses, d_options, d_stateIn, L.sc, stream));
        const int chains = sh.B * (s == 0 ? 1 : fpe::beam_live(sh, s - 1)) * sh.M;
        const fpe::PlanChain chain{L.sc.strides, (s == 0 && !d_stateIn) ? nullptr : L.sc.stateIn, L.sc.stateOut};
        fpe_plan_out cand = L.sc.cand;
        if (s > 0) cand.stance = nullptr;  // (a checked beam's start feet: segment 0's alone)
        int rc = launch_plan(h, cp, L.sc.poses, chains, sh.k, cand, stream, chain);
        if (rc != FPE_OK) return rc;
        if (check) {
            rc = beam_check_prune(*check, cp, bc, L, s, stream);
            if (rc != FPE_OK) return rc;
        } else {
            FPE_HIP(fpe::launch_beam_prune(bc, sh, s, L.sc, stream));
        }
    }
    if (check) return beam_check_trace(*check, L, stream);
    FPE_HIP(fpe::launch_beam_trace(sh, L.sc, L.out, stream));
    return FPE_OK;
}

int beam_device_call(fpe_handle h, const fpe_params* params, const fpe_beam_params* beam, BeamCheckCall* check, const fpe_pose* d_poses,
                     const fpe_plan_state* d_state_in, int32_t B, const fpe_stride* d_options, int32_t M, const fpe_beam_out* d_out,
                     void* stream);
int beam_host_call(fpe_handle h, const fpe_params* params, const fpe_beam_params* beam, BeamCheckCall* check, const fpe_pose* poses,
                   const fpe_plan_state* state_in, const double* start_feet, int32_t B, const fpe_stride* options, int32_t M,
                   const fpe_beam_out* out);
}  // namespace

int fpe_plan_beam_device(fpe_handle h, const fpe_params* params, const fpe_beam_params* beam, const fpe_pose* d_poses,
                         const fpe_plan_state* d_state_in, int32_t B, const fpe_stride* d_options, int32_t M, const fpe_beam_out* d_out,
                         void* stream) {
    return beam_device_call(h, params, beam, nullptr, d_poses, d_state_in, B, d_options, M, d_out, stream);
}

namespace {
// The device form of every beam call; check's arguments that need no map are checked by the caller's entry point.
int beam_device_call(fpe_handle h, const fpe_params* params, const fpe_beam_params* beam, BeamCheckCall* check, const fpe_pose* d_poses,
                     const fpe_plan_state* d_state_in, int32_t B, const fpe_stride* d_options, int32_t M, const fpe_beam_out* d_out,
                     void* stream) {
    BeamLayout L{};
    fpe::BeamConsts bc;
    int rc = check_beam_args(params, beam, B, M, d_out, bc, L.sh);
    if (rc != FPE_OK) return rc;
    if (!h || !d_poses || !d_options) return fail(FPE_E_INVALID_ARG, "null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    CallPlan cp;
    rc = prepare_call(h, params, 0.0f, cp, st, true);
    if (rc != FPE_OK) return rc;
    rc = check_strides_launchable(cp, fpe::PlanForm::Resume);  // (a refusal queues nothing: ahead of the async mark)
    if (rc != FPE_OK) return rc;
    rc = check_packed_fits(cp, d_out->products.selected_packed != nullptr);
    if (rc != FPE_OK) return rc;
    const bool wantStance = check && beam_check_wants_stance(*check, d_state_in != nullptr);
    if (check) {
        rc = beam_check_map(h, *check, *params, cp);
        if (rc == FPE_OK) rc = beam_check_planes(*check, *params, cp, st);
        if (rc != FPE_OK) return rc;
        beam_check_mark_async(*check);
    }
    ArenaCursor sizes;
    beam_layout(L, sizes, *d_out, false, wantStance);
    if (check) beam_check_layout(*check, L, sizes, false);
    mark_async_launch(cp);
    return with_stream_scratch(sizes.scratchBytes, st, [&](unsigned char* scratch) {
        ArenaCursor A{scratch};
        beam_layout(L, A, *d_out, false, wantStance);
        if (check) beam_check_layout(*check, L, A, false);
        return run_beam(h, cp, bc, d_poses, d_options, d_state_in, L, st, check);
    });
}
}  // namespace

int fpe_plan_beam(fpe_handle h, const fpe_params* params, const fpe_beam_params* beam, const fpe_pose* poses, const fpe_plan_state* state_in,
                  int32_t B, const fpe_stride* options, int32_t M, const fpe_beam_out* out) {
    return beam_host_call(h, params, beam, nullptr, poses, state_in, nullptr, B, options, M, out);
}

namespace {
// Where a checked beam's host form finds the start feet it staged (device pointer; beam_check_prune reads it), and its look at
// their values (the swing's segment ends: finite, within 1e6 m)
void beam_check_set_start_feet(BeamCheckCall& bc, const double* d_startFeet);
int beam_check_host_feet(const BeamCheckCall& bc, const double* startFeet, int32_t B);

// The host form of every beam call (as beam_device_call); start_feet: a checked beam's, staged behind the states
int beam_host_call(fpe_handle h, const fpe_params* params, const fpe_beam_params* beam, BeamCheckCall* check, const fpe_pose* poses,
                   const fpe_plan_state* state_in, const double* start_feet, int32_t B, const fpe_stride* options, int32_t M,
                   const fpe_beam_out* out) {
    BeamLayout L{};
    fpe::BeamConsts bc;
    int rc = check_beam_args(params, beam, B, M, out, bc, L.sh);
    if (rc != FPE_OK) return rc;
    if (!h || !poses || !options) return fail(FPE_E_INVALID_ARG, "null argument");
    float maxRadius = 0.0f;
    rc = check_host_poses(poses, B, maxRadius);
    if (rc != FPE_OK) return rc;
    rc = check_host_strides(options, M);
    if (rc != FPE_OK) return rc;
    rc = check_host_states(state_in, B, L.sh.S * L.sh.k);
    if (rc == FPE_OK && check) rc = beam_check_host_feet(*check, start_feet, B);
    if (rc != FPE_OK) return rc;
    const fpe::BeamShape want = L.sh;  // (the caller's arrays: W slots per root)
    L.sh.outStride = L.sh.slotStride;  // the arena's output block is dense: only live slots exist there
    const bool wantStance = check && beam_check_wants_stance(*check, state_in != nullptr);
    ArenaCursor sizes;
    beam_layout(L, sizes, *out, true, wantStance);
    if (check) beam_check_layout(*check, L, sizes, true);
    // both arenas: [poses | options | state_in | start_feet | outputs | scratch (device arena only)]; the inputs are read from the pinned arena
    const size_t oOptions = align256(static_cast<size_t>(B) * sizeof(fpe_pose));
    const size_t oStates = oOptions + align256(static_cast<size_t>(M) * sizeof(fpe_stride));
    const size_t oFeet = oStates + (state_in ? align256(static_cast<size_t>(B) * sizeof(fpe_plan_state)) : 0);
    const size_t szIn = oFeet + (start_feet ? align256(static_cast<size_t>(B) * 12 * sizeof(double)) : 0);
    HostCall hc(h);
    CallCtx& cx = hc.cx;
    unsigned char* in = nullptr;
    rc = open_batch_call(h, hc, params, maxRadius, szIn + sizes.outBytes + sizes.scratchBytes, out->products.selected_packed != nullptr,
                         fpe::PlanForm::Resume, in);
    if (rc != FPE_OK) return rc;
    if (check) {
        rc = beam_check_map(h, *check, *params, hc.cp);
        if (rc == FPE_OK) rc = beam_check_planes(*check, *params, hc.cp, cx.stream);
        if (rc != FPE_OK) return rc;
    }
    stage_batch_inputs(cx.pinned, 0, poses, nullptr, B, oStates, state_in);
    std::memcpy(cx.pinned + oOptions, options, static_cast<size_t>(M) * sizeof(fpe_stride));
    if (start_feet) {
        std::memcpy(cx.pinned + oFeet, start_feet, static_cast<size_t>(B) * 12 * sizeof(double));
        beam_check_set_start_feet(*check, reinterpret_cast<const double*>(in + oFeet));
    }
    ArenaCursor A{cx.dev + szIn + sizes.outBytes, cx.dev + szIn, szIn};
    beam_layout(L, A, *out, true, wantStance);
    if (check) beam_check_layout(*check, L, A, true);
    rc = run_beam(h, hc.cp, bc, reinterpret_cast<const fpe_pose*>(in), reinterpret_cast<const fpe_stride*>(in + oOptions),
                  state_in ? reinterpret_cast<const fpe_plan_state*>(in + oStates) : nullptr, L, cx.stream, check);
    if (rc != FPE_OK) return rc;
    if (L.sh.outStride == want.outStride) return copy_out(h, cx, A.outs, cx.dev, cx.pinned);  // a full beam: the arena's arrays are the caller's
    // an underfilled beam (M^S < W: a few slots): one transfer, then every root's live slots to the head of its W slots — the dead
    // ones are not written
    FPE_HIP(hipMemcpyAsync(cx.pinned + szIn, cx.dev + szIn, A.outBytes, hipMemcpyDeviceToHost, cx.stream));
    FPE_HIP(hipStreamSynchronize(cx.stream));
    cx.inFlight = false;
    for (int q = 0; q < A.outs.n; ++q) {
        const Seg& seg = A.outs.s[q];
        const unsigned char* src = cx.pinned + seg.off;
        if (!L.outSlot[q]) {
            std::memcpy(seg.dst, src, seg.len);
            continue;
        }
        const size_t live = L.outSlot[q] * L.sh.outStride, all = L.outSlot[q] * want.outStride;
        for (int b = 0; b < B; ++b) std::memcpy(static_cast<unsigned char*>(seg.dst) + b * all, src + b * live, live);
    }
    return FPE_OK;
}
}  // namespace

// ---- swing checks (fpe_swing_*; kernels: fpe_swing.hpp) ------------------------------------------------------------------------
int fpe_swing_limits_defaults(fpe_swing_limits* out) {
    if (!out) return fail(FPE_E_INVALID_ARG, "null argument");
    std::memset(out, 0, sizeof(*out));
    out->max_lift = out->max_rise = out->max_length = std::numeric_limits<double>::infinity();
    return FPE_OK;
}

namespace {
// The limits of a swing call as the kernels take them (limits NULL: the defaults), checked; the default radius resolved.
int swing_consts(const fpe_params* params, const fpe_swing_limits* limits, fpe::SwingConsts& sc) {
    if (!params) return fail(FPE_E_INVALID_ARG, "null handle or params");
    fpe_swing_limits def;
    if (!limits) {
        fpe_swing_limits_defaults(&def);
        limits = &def;
    }
    if (limits->reserved != 0) return fail(FPE_E_INVALID_ARG, "fpe_swing_limits.reserved must be 0");
    if (std::isnan(limits->max_lift) || std::isnan(limits->max_rise) || std::isnan(limits->max_length))
        return fail(FPE_E_INVALID_ARG, "swing limits must not be NaN");
    const float r = limits->radius > 0.0f ? limits->radius : params->footRadius;
    if (!std::isfinite(limits->radius) || !std::isfinite(r) || r > FPE_SWING_MAX_RADIUS)
        return fail(FPE_E_INVALID_ARG, "swing radius must be finite and at most FPE_SWING_MAX_RADIUS");
    sc = fpe::SwingConsts{limits->max_lift, limits->max_rise, limits->max_length * limits->max_length, r, 0};
    return FPE_OK;
}
int check_swing_map(const CallPlan& cp) {
    if (!fpe::swing_map_supported(cp.snap->g))
        return fail(FPE_E_UNSUPPORTED, "swing checks need a resolution of at least 1e-4 m and a map within 2e6 m of the origin");
    return FPE_OK;
}
// One segment end or start foot of a host-form call
bool swing_point_ok(const double* p) {
    for (int k = 0; k < 3; ++k)
        if (!(std::fabs(p[k]) <= 1e6)) return false;  // (NaN and infinities fail the comparison)
    return true;
}
int check_swing_shape(int32_t B, int32_t n_cycles) {
    if (B <= 0 || n_cycles <= 0 || n_cycles > 255) return fail(FPE_E_INVALID_ARG, "B and n_cycles must be in [1, ..] / [1, 255]");
    if (static_cast<int64_t>(B) * n_cycles * 4 > (1 << 30)) return fail(FPE_E_INVALID_ARG, "B * n_cycles * 4 must not exceed 2^30");
    return FPE_OK;
}
}  // namespace

int fpe_swing_segments_device(fpe_handle h, const fpe_params* params, const fpe_swing_limits* limits, const fpe_swing_query* d_queries,
                              int32_t n, fpe_swing_record* d_out, void* stream) {
    if (!d_queries || !d_out) return fail(FPE_E_INVALID_ARG, "null argument");
    if (n <= 0) return fail(FPE_E_INVALID_ARG, "n must be positive");
    fpe::SwingConsts sc;
    int rc = swing_consts(params, limits, sc);
    if (rc != FPE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    CallPlan cp;
    rc = prepare_call(h, params, 0.0f, cp, st, false);
    if (rc == FPE_OK) rc = check_swing_map(cp);
    if (rc != FPE_OK) return rc;
    mark_async_launch(cp);
    FPE_HIP(fpe::launch_swing_segments(dev_map(*cp.snap), sc, d_queries, n, d_out, st));
    return FPE_OK;
}

int fpe_swing_segments(fpe_handle h, const fpe_params* params, const fpe_swing_limits* limits, const fpe_swing_query* queries, int32_t n,
                       fpe_swing_record* out) {
    if (!queries || !out) return fail(FPE_E_INVALID_ARG, "null argument");
    if (n <= 0) return fail(FPE_E_INVALID_ARG, "n must be positive");
    fpe::SwingConsts sc;
    const int rc = swing_consts(params, limits, sc);
    if (rc != FPE_OK) return rc;
    for (int k = 0; k < n; ++k) {
        if (queries[k].reserved != 0) return fail(FPE_E_INVALID_ARG, "fpe_swing_query.reserved must be 0");
        if (!swing_point_ok(queries[k].a) || !swing_point_ok(queries[k].b)) return fail(FPE_E_INVALID_ARG, "non-finite or over-bound segment");
        if (!std::isfinite(queries[k].radius) || queries[k].radius > FPE_SWING_MAX_RADIUS) return fail(FPE_E_INVALID_ARG, "bad segment radius");
    }
    return query_round_trip(h, params, 0.0f, queries, n, out,
                            [&](const CallPlan& cp, const fpe_swing_query* d_q, fpe_swing_record* d_out, hipStream_t s) {
                                return fpe::launch_swing_segments(dev_map(*cp.snap), sc, d_q, n, d_out, s);
                            },
                            check_swing_map);
}

int fpe_swing_plan_device(fpe_handle h, const fpe_params* params, const fpe_swing_limits* limits, const fpe_plan_out* d_products,
                          const double* d_start_feet, int32_t B, int32_t n_cycles, const fpe_swing_out* d_out, void* stream) {
    if (!d_products || !d_out || !d_products->nominal || !d_products->cycle_ok) return fail(FPE_E_INVALID_ARG, "null argument");
    if (!d_start_feet && !d_products->stance) return fail(FPE_E_INVALID_ARG, "neither start feet nor the stance product given");
    if (!d_out->records && !d_out->summary) return fail(FPE_E_INVALID_ARG, "no swing output requested");
    fpe::SwingConsts sc;
    int rc = check_swing_shape(B, n_cycles);
    if (rc == FPE_OK) rc = swing_consts(params, limits, sc);
    if (rc != FPE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    CallPlan cp;
    rc = prepare_call(h, params, 0.0f, cp, st, false);
    if (rc == FPE_OK) rc = check_swing_map(cp);
    if (rc != FPE_OK) return rc;
    mark_async_launch(cp);
    const double* feet = d_start_feet ? d_start_feet : d_products->stance;
    if (d_out->records) {
        FPE_HIP(fpe::launch_swing_plan(dev_map(*cp.snap), sc, d_products->nominal, d_products->cycle_ok, feet, B, n_cycles, d_out->records,
                                       d_out->summary, st));
        return FPE_OK;
    }
    // the summary alone: its records live in stream-ordered scratch
    return with_stream_scratch(static_cast<size_t>(B) * n_cycles * 4 * sizeof(fpe_swing_record), st, [&](unsigned char* scratch) {
        FPE_HIP(fpe::launch_swing_plan(dev_map(*cp.snap), sc, d_products->nominal, d_products->cycle_ok, feet, B, n_cycles,
                                       reinterpret_cast<fpe_swing_record*>(scratch), d_out->summary, st));
        return static_cast<int>(FPE_OK);
    });
}

namespace {
// Where everything a plan-and-check call touches on the device lives: the plan's products — the requested ones in the output block,
// what the check reads besides (nominal, cycle_ok, stance) in scratch, null for the rest — then the records (scratch when only the
// summary is wanted) and the summary.
struct SwingLayout {
    int32_t B, n;
    fpe_plan_out plan;
    fpe_swing_record* records;
    fpe_swing_summary* summary;
};
static_assert(kPlanProducts + 2 <= kMaxSegs, "SegList holds a plan-and-check call's outputs");
void swing_layout(SwingLayout& L, ArenaCursor& A, const fpe_plan_out* want, const fpe_swing_out& so) {
    const bool reads[kPlanProducts] = {true, false, false, true, true, false, false, false};  // swing_segments_kernel<true>'s inputs
    const size_t B = static_cast<size_t>(L.B), n = static_cast<size_t>(L.n);
    void* const* wanted = want ? slots(*want) : nullptr;
    for (int k = 0; k < kPlanProducts; ++k)
        slots(L.plan)[k] = (wanted && wanted[k]) ? A.out(wanted[k], product_bytes(k, B, n)) : (reads[k] ? A.take(product_bytes(k, B, n)) : nullptr);
    const size_t szRec = B * n * 4 * sizeof(fpe_swing_record);
    L.records = static_cast<fpe_swing_record*>(so.records ? A.out(so.records, szRec) : A.take(szRec));
    L.summary = static_cast<fpe_swing_summary*>(so.summary ? A.out(so.summary, B * sizeof(fpe_swing_summary)) : nullptr);
}
}  // namespace

int fpe_swing_plan(fpe_handle h, const fpe_params* params, const fpe_swing_limits* limits, const fpe_pose* poses, const fpe_stride* strides,
                   int32_t B, int32_t n_cycles, const fpe_plan_out* products, const fpe_swing_out* out) {
    if (!h || !poses || !out) return fail(FPE_E_INVALID_ARG, "null argument");
    if (!out->records && !out->summary) return fail(FPE_E_INVALID_ARG, "no swing output requested");
    fpe::SwingConsts sc;
    int rc = check_swing_shape(B, n_cycles);
    if (rc == FPE_OK) rc = swing_consts(params, limits, sc);
    if (rc != FPE_OK) return rc;
    float maxRadius = 0.0f;
    rc = check_host_poses(poses, B, maxRadius);
    if (rc == FPE_OK) rc = check_host_strides(strides, B);
    if (rc != FPE_OK) return rc;
    SwingLayout L{};
    L.B = B, L.n = n_cycles;
    ArenaCursor sizes;
    swing_layout(L, sizes, products, *out);
    // both arenas: [poses (| strides) | outputs | scratch (device arena only)]; the inputs are read from the pinned arena, as in fpe_plan
    const size_t oStrides = align256(static_cast<size_t>(B) * sizeof(fpe_pose));
    const size_t szIn = oStrides + (strides ? align256(static_cast<size_t>(B) * sizeof(fpe_stride)) : 0);
    HostCall hc(h);
    CallCtx& cx = hc.cx;
    unsigned char* in = nullptr;
    rc = open_batch_call(h, hc, params, maxRadius, szIn + sizes.outBytes + sizes.scratchBytes, products && products->selected_packed,
                         strides ? fpe::PlanForm::Stride : fpe::PlanForm::Plain, in);
    if (rc == FPE_OK) rc = check_swing_map(hc.cp);
    if (rc != FPE_OK) return rc;
    stage_batch_inputs(cx.pinned, oStrides, poses, strides, B);
    ArenaCursor A{cx.dev + szIn + sizes.outBytes, cx.dev + szIn, szIn};
    swing_layout(L, A, products, *out);
    // the plan through the plan runner, then the check behind it on the same stream and the same snapshot
    rc = launch_plan(h, hc.cp, reinterpret_cast<const fpe_pose*>(in), B, n_cycles, L.plan, cx.stream,
                     {strides ? reinterpret_cast<const fpe_stride*>(in + oStrides) : nullptr});
    if (rc != FPE_OK) return rc;
    FPE_HIP(fpe::launch_swing_plan(dev_map(*hc.cp.snap), sc, L.plan.nominal, L.plan.cycle_ok, L.plan.stance, B, n_cycles, L.records, L.summary,
                                   cx.stream));
    return copy_out(h, cx, A.outs, cx.dev, cx.pinned);
}

// ---- trunk checks (fpe_trunk_*; kernels: fpe_trunk.hpp) ------------------------------------------------------------------------
int fpe_trunk_limits_defaults(fpe_trunk_limits* out) {
    if (!out) return fail(FPE_E_INVALID_ARG, "null argument");
    std::memset(out, 0, sizeof(*out));
    out->min_clearance = -std::numeric_limits<double>::infinity();
    out->max_slope_x = out->max_slope_y = std::numeric_limits<double>::infinity();
    return FPE_OK;
}

namespace {
// The limits of a trunk call as the kernels take them (limits NULL: the defaults), checked; the default box resolved.
int trunk_consts(const fpe_params* params, const fpe_trunk_limits* limits, fpe::TrunkConsts& tc) {
    if (!params) return fail(FPE_E_INVALID_ARG, "null handle or params");
    fpe_trunk_limits def;
    if (!limits) {
        fpe_trunk_limits_defaults(&def);
        limits = &def;
    }
    if (limits->reserved[0] != 0 || limits->reserved[1] != 0) return fail(FPE_E_INVALID_ARG, "fpe_trunk_limits.reserved must be 0");
    if (std::isnan(limits->min_clearance) || std::isnan(limits->max_slope_x) || std::isnan(limits->max_slope_y) ||
        std::isnan(limits->half_length) || std::isnan(limits->half_width))
        return fail(FPE_E_INVALID_ARG, "trunk limits must not be NaN");
    if (!(std::fabs(limits->ride_height) <= 1e6)) return fail(FPE_E_INVALID_ARG, "ride_height must be finite and within +-1e6");
    const double hx = limits->half_length > 0.0f ? static_cast<double>(limits->half_length) : 0.5 * static_cast<double>(params->length);
    const double hy = limits->half_width > 0.0f ? static_cast<double>(limits->half_width) : 0.5 * static_cast<double>(params->width);
    for (double v : {hx, hy})
        if (!std::isfinite(v) || !(v > 0.0) || v > static_cast<double>(FPE_TRUNK_MAX_HALF_EXTENT))
            return fail(FPE_E_INVALID_ARG, "the default trunk half extents must be finite, positive and at most FPE_TRUNK_MAX_HALF_EXTENT");
    tc = fpe::TrunkConsts{limits->min_clearance, limits->max_slope_x, limits->max_slope_y, limits->ride_height, hx, hy};
    return FPE_OK;
}
// What needs the call's snapshot: the maps the enumeration is proven on, and the default box against the cell cap
int check_trunk_map(const CallPlan& cp, const fpe::TrunkConsts& tc) {
    if (!fpe::swing_map_supported(cp.snap->g))
        return fail(FPE_E_UNSUPPORTED, "trunk checks need a resolution of at least 1e-4 m and a map within 2e6 m of the origin");
    if (!fpe::trunk_box_supported(tc.defaultHx, tc.defaultHy, cp.snap->g.res))
        return fail(FPE_E_UNSUPPORTED, "the default trunk box exceeds FPE_TRUNK_MAX_CELLS cells at this resolution");
    return FPE_OK;
}
int check_trunk_shape(int32_t B, int32_t n_cycles) {
    if (B <= 0 || n_cycles <= 0 || n_cycles > 255) return fail(FPE_E_INVALID_ARG, "B and n_cycles must be in [1, ..] / [1, 255]");
    if (static_cast<int64_t>(B) * n_cycles > (1 << 30)) return fail(FPE_E_INVALID_ARG, "B * n_cycles must not exceed 2^30");
    return FPE_OK;
}
}  // namespace

int fpe_trunk_stances_device(fpe_handle h, const fpe_params* params, const fpe_trunk_limits* limits, const fpe_trunk_query* d_queries,
                             int32_t n, fpe_trunk_record* d_out, void* stream) {
    if (!d_queries || !d_out) return fail(FPE_E_INVALID_ARG, "null argument");
    if (n <= 0) return fail(FPE_E_INVALID_ARG, "n must be positive");
    fpe::TrunkConsts tc;
    int rc = trunk_consts(params, limits, tc);
    if (rc != FPE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    CallPlan cp;
    rc = prepare_call(h, params, 0.0f, cp, st, false);
    if (rc == FPE_OK) rc = check_trunk_map(cp, tc);
    if (rc != FPE_OK) return rc;
    mark_async_launch(cp);
    FPE_HIP(fpe::launch_trunk_stances(dev_map(*cp.snap), tc, d_queries, n, d_out, st));
    return FPE_OK;
}

int fpe_trunk_stances(fpe_handle h, const fpe_params* params, const fpe_trunk_limits* limits, const fpe_trunk_query* queries, int32_t n,
                      fpe_trunk_record* out) {
    if (!queries || !out) return fail(FPE_E_INVALID_ARG, "null argument");
    if (n <= 0) return fail(FPE_E_INVALID_ARG, "n must be positive");
    fpe::TrunkConsts tc;
    const int rc = trunk_consts(params, limits, tc);
    if (rc != FPE_OK) return rc;
    for (int k = 0; k < n; ++k)
        if (queries[k].reserved[0] != 0 || queries[k].reserved[1] != 0) return fail(FPE_E_INVALID_ARG, "fpe_trunk_query.reserved must be 0");
    return query_round_trip(h, params, 0.0f, queries, n, out,
                            [&](const CallPlan& cp, const fpe_trunk_query* d_q, fpe_trunk_record* d_out, hipStream_t s) {
                                return fpe::launch_trunk_stances(dev_map(*cp.snap), tc, d_q, n, d_out, s);
                            },
                            [&](const CallPlan& cp) {
                                const int rm = check_trunk_map(cp, tc);
                                if (rm != FPE_OK) return rm;
                                for (int k = 0; k < n; ++k)  // (the cell cap is in cells: it needs the snapshot's resolution)
                                    if (fpe::trunk_stance_refused(tc, queries[k], cp.snap->g.res))
                                        return fail(FPE_E_INVALID_ARG, "non-finite or over-bound stance, half extent, box or slope");
                                return static_cast<int>(FPE_OK);
                            });
}

int fpe_trunk_plan_device(fpe_handle h, const fpe_params* params, const fpe_trunk_limits* limits, const fpe_plan_out* d_products,
                          int32_t B, int32_t n_cycles, const fpe_trunk_out* d_out, void* stream) {
    if (!d_products || !d_out || !d_products->nominal || !d_products->cycle_ok) return fail(FPE_E_INVALID_ARG, "null argument");
    if (!d_out->records && !d_out->summary) return fail(FPE_E_INVALID_ARG, "no trunk output requested");
    fpe::TrunkConsts tc;
    int rc = check_trunk_shape(B, n_cycles);
    if (rc == FPE_OK) rc = trunk_consts(params, limits, tc);
    if (rc != FPE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    CallPlan cp;
    rc = prepare_call(h, params, 0.0f, cp, st, false);
    if (rc == FPE_OK) rc = check_trunk_map(cp, tc);
    if (rc != FPE_OK) return rc;
    mark_async_launch(cp);
    if (d_out->records) {
        FPE_HIP(fpe::launch_trunk_plan(dev_map(*cp.snap), tc, d_products->nominal, d_products->cycle_ok, B, n_cycles, d_out->records,
                                       d_out->summary, st));
        return FPE_OK;
    }
    // the summary alone: its records live in stream-ordered scratch
    return with_stream_scratch(static_cast<size_t>(B) * n_cycles * sizeof(fpe_trunk_record), st, [&](unsigned char* scratch) {
        FPE_HIP(fpe::launch_trunk_plan(dev_map(*cp.snap), tc, d_products->nominal, d_products->cycle_ok, B, n_cycles,
                                       reinterpret_cast<fpe_trunk_record*>(scratch), d_out->summary, st));
        return static_cast<int>(FPE_OK);
    });
}

namespace {
// Where everything a plan-and-check call touches on the device lives: the plan's products — the requested ones in the output block,
// what the check reads besides (nominal, cycle_ok) in scratch, null for the rest — then the records (scratch when only the summary is
// wanted) and the summary.
struct TrunkLayout {
    int32_t B, n;
    fpe_plan_out plan;
    fpe_trunk_record* records;
    fpe_trunk_summary* summary;
};
void trunk_layout(TrunkLayout& L, ArenaCursor& A, const fpe_plan_out* want, const fpe_trunk_out& to) {
    const bool reads[kPlanProducts] = {true, false, false, true, false, false, false, false};  // trunk_stances_kernel<true>'s inputs
    const size_t B = static_cast<size_t>(L.B), n = static_cast<size_t>(L.n);
    void* const* wanted = want ? slots(*want) : nullptr;
    for (int k = 0; k < kPlanProducts; ++k)
        slots(L.plan)[k] = (wanted && wanted[k]) ? A.out(wanted[k], product_bytes(k, B, n)) : (reads[k] ? A.take(product_bytes(k, B, n)) : nullptr);
    const size_t szRec = B * n * sizeof(fpe_trunk_record);
    L.records = static_cast<fpe_trunk_record*>(to.records ? A.out(to.records, szRec) : A.take(szRec));
    L.summary = static_cast<fpe_trunk_summary*>(to.summary ? A.out(to.summary, B * sizeof(fpe_trunk_summary)) : nullptr);
}
}  // namespace

int fpe_trunk_plan(fpe_handle h, const fpe_params* params, const fpe_trunk_limits* limits, const fpe_pose* poses, const fpe_stride* strides,
                   int32_t B, int32_t n_cycles, const fpe_plan_out* products, const fpe_trunk_out* out) {
    if (!h || !poses || !out) return fail(FPE_E_INVALID_ARG, "null argument");
    if (!out->records && !out->summary) return fail(FPE_E_INVALID_ARG, "no trunk output requested");
    fpe::TrunkConsts tc;
    int rc = check_trunk_shape(B, n_cycles);
    if (rc == FPE_OK) rc = trunk_consts(params, limits, tc);
    if (rc != FPE_OK) return rc;
    float maxRadius = 0.0f;
    rc = check_host_poses(poses, B, maxRadius);
    if (rc == FPE_OK) rc = check_host_strides(strides, B);
    if (rc != FPE_OK) return rc;
    TrunkLayout L{};
    L.B = B, L.n = n_cycles;
    ArenaCursor sizes;
    trunk_layout(L, sizes, products, *out);
    // both arenas: [poses (| strides) | outputs | scratch (device arena only)]; the inputs are read from the pinned arena, as in fpe_plan
    const size_t oStrides = align256(static_cast<size_t>(B) * sizeof(fpe_pose));
    const size_t szIn = oStrides + (strides ? align256(static_cast<size_t>(B) * sizeof(fpe_stride)) : 0);
    HostCall hc(h);
    CallCtx& cx = hc.cx;
    unsigned char* in = nullptr;
    rc = open_batch_call(h, hc, params, maxRadius, szIn + sizes.outBytes + sizes.scratchBytes, products && products->selected_packed,
                         strides ? fpe::PlanForm::Stride : fpe::PlanForm::Plain, in);
    if (rc == FPE_OK) rc = check_trunk_map(hc.cp, tc);
    if (rc != FPE_OK) return rc;
    stage_batch_inputs(cx.pinned, oStrides, poses, strides, B);
    ArenaCursor A{cx.dev + szIn + sizes.outBytes, cx.dev + szIn, szIn};
    trunk_layout(L, A, products, *out);
    // the plan through the plan runner, then the check behind it on the same stream and the same snapshot
    rc = launch_plan(h, hc.cp, reinterpret_cast<const fpe_pose*>(in), B, n_cycles, L.plan, cx.stream,
                     {strides ? reinterpret_cast<const fpe_stride*>(in + oStrides) : nullptr});
    if (rc != FPE_OK) return rc;
    FPE_HIP(fpe::launch_trunk_plan(dev_map(*hc.cp.snap), tc, L.plan.nominal, L.plan.cycle_ok, B, n_cycles, L.records, L.summary, cx.stream));
    return copy_out(h, cx, A.outs, cx.dev, cx.pinned);
}

// ---- edge margin (fpe_margin_*; kernels: fpe_margin.hpp) -----------------------------------------------------------------------
int fpe_margin_params_defaults(fpe_margin_params* out) {
    if (!out) return fail(FPE_E_INVALID_ARG, "null argument");
    std::memset(out, 0, sizeof(*out));
    out->classes = FPE_MARGIN_LOW_CANDIDATE | FPE_MARGIN_UNKNOWN | FPE_MARGIN_OFF_MAP;
    out->reach_cells = 8;
    return FPE_OK;
}

namespace {
// The parameters of a margin call (mp NULL: the defaults), checked; what needs no map.
int margin_params(const fpe_margin_params* mp, fpe_margin_params& r) {
    if (!mp) {
        fpe_margin_params_defaults(&r);
        return FPE_OK;
    }
    r = *mp;
    if (r.classes < 1 || r.classes > 15) return fail(FPE_E_INVALID_ARG, "fpe_margin_params.classes must be in 1..15");
    if (r.reach_cells < 1 || r.reach_cells > FPE_MARGIN_MAX_CELLS)
        return fail(FPE_E_INVALID_ARG, "fpe_margin_params.reach_cells must be in 1..FPE_MARGIN_MAX_CELLS");
    if (r.reserved[0] != 0 || r.reserved[1] != 0) return fail(FPE_E_INVALID_ARG, "fpe_margin_params.reserved must be 0");
    if (!std::isfinite(r.min_margin) || r.min_margin < 0.0) return fail(FPE_E_INVALID_ARG, "min_margin must be finite and >= 0");
    return FPE_OK;
}
// What needs the call's snapshot: the limit against the reach, and the kernels' constants
int margin_consts(const fpe_margin_params& r, const fpe::MapGeom& g, fpe::MarginConsts& mc) {
    const double res2 = g.res * g.res, mm2 = r.min_margin * r.min_margin;
    if (mm2 > static_cast<double>(r.reach_cells * r.reach_cells) * res2)
        return fail(FPE_E_UNSUPPORTED, "min_margin lies beyond reach_cells at this resolution: the reach cannot decide the limit");
    mc = fpe::MarginConsts{r.classes, r.reach_cells, res2, mm2};
    return FPE_OK;
}
int check_margin_shape(int32_t B, int32_t n_cycles) {
    if (B <= 0 || n_cycles <= 0 || n_cycles > 255) return fail(FPE_E_INVALID_ARG, "B and n_cycles must be in [1, ..] / [1, 255]");
    if (static_cast<int64_t>(B) * n_cycles * 4 > (1 << 30)) return fail(FPE_E_INVALID_ARG, "B * n_cycles * 4 must not exceed 2^30");
    return FPE_OK;
}
// The planes of the call's threshold pair on cp.snap, built on `stream` on first use (the lookup of prepare_call)
int margin_planes(const fpe_params& params, CallPlan& cp, hipStream_t stream) {
    return acquire_mask(*cp.snap, params.defaultFootholdThreshold, params.candidateFootholdThreshold, stream, cp);
}
// Every form but fpe_margin_plan: the checks, the snapshot current at entry, (dense: the region,) the constants, the planes; `stream`
// ordered after the snapshot's upload and the planes' build.  queries (host; may be null): the n cells of a host form, each checked
// against the snapshot's size.  Nothing is queued ahead of a refusal.
int prepare_margin(fpe_engine* h, const fpe_params* params, const fpe_margin_params* mp, const int32_t roi[4], fpe::FootmapRoi* r,
                   CallPlan& cp, fpe::MarginConsts& mc, hipStream_t stream, const fpe_margin_query* queries = nullptr, int32_t n = 0) {
    if (!h || !params) return fail(FPE_E_INVALID_ARG, "null handle or params");
    fpe_margin_params q;
    int rc = margin_params(mp, q);
    if (rc != FPE_OK) return rc;
    rc = fpe::validate_params(*params);
    if (rc != FPE_OK) return fail(rc, "non-finite or negative parameter");
    {
        std::lock_guard<std::mutex> lk(h->mu);
        cp.snap = h->map;
    }
    if (!cp.snap) return fail(FPE_E_NO_MAP, "no map uploaded");
    if (r) {
        rc = resolve_roi(roi, cp.snap->g, *r);
        if (rc != FPE_OK) return rc;
    }
    rc = margin_consts(q, cp.snap->g, mc);
    if (rc != FPE_OK) return rc;
    for (int32_t k = 0; queries && k < n; ++k)
        if (fpe::margin_query_refused(cp.snap->g.rows, cp.snap->g.cols, queries[k]))
            return fail(FPE_E_INVALID_ARG, "a query cell lies FPE_PACKED_BIAS cells or more outside the map");
    FPE_HIP(hipSetDevice(h->device));
    FPE_HIP(cp.snap->wait_ready(stream));
    return margin_planes(*params, cp, stream);
}
}  // namespace

int fpe_margin_map_device(fpe_handle h, const fpe_params* params, const fpe_margin_params* mp, const int32_t roi[4],
                          const fpe_margin_map_out* d_out, void* stream) {
    if (!d_out) return fail(FPE_E_INVALID_ARG, "null argument");
    if (!d_out->dist_sq && !d_out->nearest) return fail(FPE_E_INVALID_ARG, "no output requested");
    hipStream_t st = static_cast<hipStream_t>(stream);
    CallPlan cp;
    fpe::FootmapRoi r{};
    fpe::MarginConsts mc;
    const int rc = prepare_margin(h, params, mp, roi, &r, cp, mc, st);
    if (rc != FPE_OK) return rc;
    mark_async_launch(cp);
    FPE_HIP(fpe::launch_margin_map(cp.bits, cp.snap->g, mc, r, d_out->dist_sq, d_out->nearest, st));
    return FPE_OK;
}

int fpe_margin_map(fpe_handle h, const fpe_params* params, const fpe_margin_params* mp, const int32_t roi[4], const fpe_margin_map_out* out) {
    if (!out) return fail(FPE_E_INVALID_ARG, "null argument");
    if (!out->dist_sq && !out->nearest) return fail(FPE_E_INVALID_ARG, "no output requested");
    if (!h) return fail(FPE_E_INVALID_ARG, "null handle or params");
    HostCall hc(h);
    CallPlan& cp = hc.cp;
    CallCtx& cx = hc.cx;
    FPE_HIP(hipSetDevice(h->device));
    FPE_HIP(cx.reserve(0));  // the stream
    fpe::FootmapRoi r{};
    fpe::MarginConsts mc;
    const int rc = prepare_margin(h, params, mp, roi, &r, cp, mc, cx.stream);
    if (rc != FPE_OK) return rc;
    const size_t n = static_cast<size_t>(r.nr) * r.nc;
    const HostProduct prod[2] = {{out->dist_sq, n * sizeof(uint16_t)}, {out->nearest, n * 2}};
    return stage_products(cx, prod, [&](unsigned char* const* d, hipStream_t s) {
        return fpe::launch_margin_map(cp.bits, cp.snap->g, mc, r, reinterpret_cast<uint16_t*>(d[0]), reinterpret_cast<int8_t*>(d[1]), s);
    });
}

int fpe_margin_cells_device(fpe_handle h, const fpe_params* params, const fpe_margin_params* mp, const fpe_margin_query* d_queries,
                            int32_t n, fpe_margin_record* d_out, void* stream) {
    if (!d_queries || !d_out) return fail(FPE_E_INVALID_ARG, "null argument");
    if (n <= 0) return fail(FPE_E_INVALID_ARG, "n must be positive");
    hipStream_t st = static_cast<hipStream_t>(stream);
    CallPlan cp;
    fpe::MarginConsts mc;
    const int rc = prepare_margin(h, params, mp, nullptr, nullptr, cp, mc, st);
    if (rc != FPE_OK) return rc;
    mark_async_launch(cp);
    FPE_HIP(fpe::launch_margin_cells(cp.bits, cp.snap->g, mc, d_queries, n, d_out, st));
    return FPE_OK;
}

int fpe_margin_cells(fpe_handle h, const fpe_params* params, const fpe_margin_params* mp, const fpe_margin_query* queries, int32_t n,
                     fpe_margin_record* out) {
    if (!queries || !out) return fail(FPE_E_INVALID_ARG, "null argument");
    if (n <= 0) return fail(FPE_E_INVALID_ARG, "n must be positive");
    if (!h) return fail(FPE_E_INVALID_ARG, "null handle or params");
    // n queries up, n records back, both through the context's arenas (as query_round_trip, behind this family's prepare)
    const size_t nQ = static_cast<size_t>(n) * sizeof(fpe_margin_query), nO = static_cast<size_t>(n) * sizeof(fpe_margin_record);
    const size_t szQ = align256(nQ);
    HostCall hc(h);
    CallPlan& cp = hc.cp;
    CallCtx& cx = hc.cx;
    FPE_HIP(hipSetDevice(h->device));
    FPE_HIP(cx.reserve(szQ + align256(nO)));
    fpe::MarginConsts mc;
    cx.inFlight = true;
    const int rc = prepare_margin(h, params, mp, nullptr, nullptr, cp, mc, cx.stream, queries, n);
    if (rc != FPE_OK) return rc;
    std::memcpy(cx.pinned, queries, nQ);
    FPE_HIP(hipMemcpyAsync(cx.dev, cx.pinned, nQ, hipMemcpyHostToDevice, cx.stream));
    FPE_HIP(fpe::launch_margin_cells(cp.bits, cp.snap->g, mc, reinterpret_cast<const fpe_margin_query*>(cx.dev), n,
                                     reinterpret_cast<fpe_margin_record*>(cx.dev + szQ), cx.stream));
    FPE_HIP(hipMemcpyAsync(cx.pinned + szQ, cx.dev + szQ, nO, hipMemcpyDeviceToHost, cx.stream));
    FPE_HIP(hipStreamSynchronize(cx.stream));
    cx.inFlight = false;
    std::memcpy(out, cx.pinned + szQ, nO);
    return FPE_OK;
}

int fpe_margin_plan_device(fpe_handle h, const fpe_params* params, const fpe_margin_params* mp, const fpe_plan_out* d_products, int32_t B,
                           int32_t n_cycles, const fpe_margin_out* d_out, void* stream) {
    if (!d_products || !d_out || !d_products->nominal) return fail(FPE_E_INVALID_ARG, "null argument");
    if (!d_out->records && !d_out->summary) return fail(FPE_E_INVALID_ARG, "no margin output requested");
    int rc = check_margin_shape(B, n_cycles);
    if (rc != FPE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    CallPlan cp;
    fpe::MarginConsts mc;
    rc = prepare_margin(h, params, mp, nullptr, nullptr, cp, mc, st);
    if (rc != FPE_OK) return rc;
    mark_async_launch(cp);
    if (d_out->records) {
        FPE_HIP(fpe::launch_margin_plan(cp.bits, cp.snap->g, mc, d_products->nominal, B, n_cycles, d_out->records, d_out->summary, st));
        return FPE_OK;
    }
    // the summary alone: its records live in stream-ordered scratch
    return with_stream_scratch(static_cast<size_t>(B) * n_cycles * 4 * sizeof(fpe_margin_record), st, [&](unsigned char* scratch) {
        FPE_HIP(fpe::launch_margin_plan(cp.bits, cp.snap->g, mc, d_products->nominal, B, n_cycles,
                                        reinterpret_cast<fpe_margin_record*>(scratch), d_out->summary, st));
        return static_cast<int>(FPE_OK);
    });
}

namespace {
// Where everything a plan-and-margin call touches on the device lives, as TrunkLayout: the plan's products — the requested ones in
// the output block, what the check reads besides (nominal) in scratch, null for the rest — then the records (scratch when only the
// summary is wanted) and the summary.
struct MarginLayout {
    int32_t B, n;
    fpe_plan_out plan;
    fpe_margin_record* records;
    fpe_margin_summary* summary;
};
void margin_layout(MarginLayout& L, ArenaCursor& A, const fpe_plan_out* want, const fpe_margin_out& mo) {
    const bool reads[kPlanProducts] = {true, false, false, false, false, false, false, false};  // margin_cells_kernel<true>'s input
    const size_t B = static_cast<size_t>(L.B), n = static_cast<size_t>(L.n);
    void* const* wanted = want ? slots(*want) : nullptr;
    for (int k = 0; k < kPlanProducts; ++k)
        slots(L.plan)[k] = (wanted && wanted[k]) ? A.out(wanted[k], product_bytes(k, B, n)) : (reads[k] ? A.take(product_bytes(k, B, n)) : nullptr);
    const size_t szRec = B * n * 4 * sizeof(fpe_margin_record);
    L.records = static_cast<fpe_margin_record*>(mo.records ? A.out(mo.records, szRec) : A.take(szRec));
    L.summary = static_cast<fpe_margin_summary*>(mo.summary ? A.out(mo.summary, B * sizeof(fpe_margin_summary)) : nullptr);
}
}  // namespace

int fpe_margin_plan(fpe_handle h, const fpe_params* params, const fpe_margin_params* mp, const fpe_pose* poses, const fpe_stride* strides,
                    int32_t B, int32_t n_cycles, const fpe_plan_out* products, const fpe_margin_out* out) {
    if (!h || !params || !poses || !out) return fail(FPE_E_INVALID_ARG, "null argument");
    if (!out->records && !out->summary) return fail(FPE_E_INVALID_ARG, "no margin output requested");
    fpe_margin_params q;
    int rc = check_margin_shape(B, n_cycles);
    if (rc == FPE_OK) rc = margin_params(mp, q);
    if (rc != FPE_OK) return rc;
    float maxRadius = 0.0f;
    rc = check_host_poses(poses, B, maxRadius);
    if (rc == FPE_OK) rc = check_host_strides(strides, B);
    if (rc != FPE_OK) return rc;
    MarginLayout L{};
    L.B = B, L.n = n_cycles;
    ArenaCursor sizes;
    margin_layout(L, sizes, products, *out);
    // both arenas: [poses (| strides) | outputs | scratch (device arena only)]; the inputs are read from the pinned arena, as in fpe_plan
    const size_t oStrides = align256(static_cast<size_t>(B) * sizeof(fpe_pose));
    const size_t szIn = oStrides + (strides ? align256(static_cast<size_t>(B) * sizeof(fpe_stride)) : 0);
    CallPlan planes;  // the margin's planes: declared ahead of the lease, so released behind it (HostCall)
    HostCall hc(h);
    CallCtx& cx = hc.cx;
    unsigned char* in = nullptr;
    rc = open_batch_call(h, hc, params, maxRadius, szIn + sizes.outBytes + sizes.scratchBytes, products && products->selected_packed,
                         strides ? fpe::PlanForm::Stride : fpe::PlanForm::Plain, in);
    fpe::MarginConsts mc;
    if (rc == FPE_OK) rc = margin_consts(q, hc.cp.snap->g, mc);
    if (rc != FPE_OK) return rc;
    // the pair's planes by the same lookup the plan made (it finds the plan's set where the plan launches with one): one snapshot
    planes.snap = hc.cp.snap;
    rc = margin_planes(*params, planes, cx.stream);
    if (rc != FPE_OK) return rc;
    stage_batch_inputs(cx.pinned, oStrides, poses, strides, B);
    ArenaCursor A{cx.dev + szIn + sizes.outBytes, cx.dev + szIn, szIn};
    margin_layout(L, A, products, *out);
    // the plan through the plan runner, then the check behind it on the same stream and the same snapshot
    rc = launch_plan(h, hc.cp, reinterpret_cast<const fpe_pose*>(in), B, n_cycles, L.plan, cx.stream,
                     {strides ? reinterpret_cast<const fpe_stride*>(in + oStrides) : nullptr});
    if (rc != FPE_OK) return rc;
    FPE_HIP(fpe::launch_margin_plan(planes.bits, planes.snap->g, mc, L.plan.nominal, B, n_cycles, L.records, L.summary, cx.stream));
    return copy_out(h, cx, A.outs, cx.dev, cx.pinned);
}

// ---- checked ranking (fpe_plan_rank_checked*, fpe_check_plan_device; kernel: fpe_check.hpp) -------------------------------------
int fpe_check_params_defaults(fpe_check_params* out) {
    if (!out) return fail(FPE_E_INVALID_ARG, "null argument");
    std::memset(out, 0, sizeof(*out));
    out->checks = FPE_CHECK_SWING | FPE_CHECK_TRUNK | FPE_CHECK_MARGIN;
    out->reject = 0;
    out->w_swing_over = 10.0;
    out->w_lift = 0.0;
    out->w_trunk_bad = 10.0;
    out->w_margin_under = 1.0;
    out->w_unknown = 1.0;
    fpe_swing_limits_defaults(&out->swing);
    fpe_trunk_limits_defaults(&out->trunk);
    fpe_margin_params_defaults(&out->margin);
    return FPE_OK;
}

namespace {
// The check stage of one call: what the caller asked for, the kernel's argument block as the checks below fill it in, and the
// margin's planes (a CallPlan of their own on the call's snapshot, as in fpe_margin_plan; the object outlives the call's lease).
struct CheckCall {
    fpe_check_out want{};       // the caller's arrays (null: not wanted; those of a disabled check: cleared)
    fpe_check_out out{};        // where the kernel writes them (check_call_layout)
    fpe_margin_params margin{};  // the checked margin block
    CallPlan planes;
    fpe::CheckStage stage{};
};

// Arguments of a check stage that need no map (checks NULL: the defaults): the bits, the weights, and each ENABLED check's block
// through the host function of its own family; a disabled check's block is not read.
int check_check_args(const fpe_params* params, const fpe_check_params* checks, const fpe_check_out* out, CheckCall& cc) {
    if (!params) return fail(FPE_E_INVALID_ARG, "null handle or params");
    fpe_check_params def;
    if (!checks) {
        fpe_check_params_defaults(&def);
        checks = &def;
    }
    constexpr uint32_t kAll = FPE_CHECK_SWING | FPE_CHECK_TRUNK | FPE_CHECK_MARGIN;
    const uint32_t on = checks->checks;
    if (on & ~kAll) return fail(FPE_E_INVALID_ARG, "fpe_check_params.checks holds bits outside SWING | TRUNK | MARGIN");
    if (checks->reject & ~(on | (on ? FPE_CHECK_UNKNOWN : 0u)))
        return fail(FPE_E_INVALID_ARG, "fpe_check_params.reject must be a subset of checks | (checks ? UNKNOWN : 0)");
    const double w[5] = {checks->w_swing_over, checks->w_lift, checks->w_trunk_bad, checks->w_margin_under, checks->w_unknown};
    for (double v : w)
        if (!std::isfinite(v)) return fail(FPE_E_INVALID_ARG, "check weights must be finite");
    uint64_t reservedBits;
    std::memcpy(&reservedBits, &checks->reserved, sizeof(reservedBits));
    if (reservedBits != 0) return fail(FPE_E_INVALID_ARG, "fpe_check_params.reserved must be +0.0");
    fpe::CheckArgs& a = cc.stage.a;
    a.checks = on, a.reject = checks->reject;
    a.wSwingOver = w[0], a.wLift = w[1], a.wTrunkBad = w[2], a.wMarginUnder = w[3], a.wUnknown = w[4];
    int rc = FPE_OK;
    if (on & FPE_CHECK_SWING) rc = swing_consts(params, &checks->swing, a.sc);
    if (rc == FPE_OK && (on & FPE_CHECK_TRUNK)) rc = trunk_consts(params, &checks->trunk, a.tc);
    if (rc == FPE_OK && (on & FPE_CHECK_MARGIN)) rc = margin_params(&checks->margin, cc.margin);
    if (rc != FPE_OK) return rc;
    if (out) cc.want = *out;
    if (!(on & FPE_CHECK_SWING)) cc.want.swing = nullptr;
    if (!(on & FPE_CHECK_TRUNK)) cc.want.trunk = nullptr;
    if (!(on & FPE_CHECK_MARGIN)) cc.want.margin = nullptr;
    return FPE_OK;
}

int check_call_map(CheckCall& cc, const CallPlan& cp) {
    fpe::CheckArgs& a = cc.stage.a;
    int rc = FPE_OK;
    if (a.checks & FPE_CHECK_SWING) rc = check_swing_map(cp);
    if (rc == FPE_OK && (a.checks & FPE_CHECK_TRUNK)) rc = check_trunk_map(cp, a.tc);
    if (rc == FPE_OK && (a.checks & FPE_CHECK_MARGIN)) {
        rc = margin_consts(cc.margin, cp.snap->g, a.mc);
        a.marginLanesLog2 = fpe::margin_lanes_log2(cc.margin.reach_cells);
    }
    return rc;
}

// The pair's planes on the call's snapshot by the lookup the plan made, built on `stream` on first use (as fpe_margin_plan)
int check_call_planes(CheckCall& cc, const fpe_params& params, const CallPlan& cp, hipStream_t stream) {
    if (!(cc.stage.a.checks & FPE_CHECK_MARGIN)) return FPE_OK;
    cc.planes.snap = cp.snap;
    return margin_planes(params, cc.planes, stream);
}

void check_call_mark_async(const CheckCall& cc) {
    if (cc.planes.snap) mark_async_launch(cc.planes);
}

void check_call_layout(CheckCall& cc, ArenaCursor& A, int32_t B, bool hostForm) {
    const size_t n = static_cast<size_t>(B);
    const auto out = [&](void* dst, size_t bytes) { return (dst && hostForm) ? A.out(dst, bytes) : dst; };
    cc.out.swing = static_cast<fpe_swing_summary*>(out(cc.want.swing, n * sizeof(fpe_swing_summary)));
    cc.out.trunk = static_cast<fpe_trunk_summary*>(out(cc.want.trunk, n * sizeof(fpe_trunk_summary)));
    cc.out.margin = static_cast<fpe_margin_summary*>(out(cc.want.margin, n * sizeof(fpe_margin_summary)));
    cc.out.base_score = static_cast<double*>(out(cc.want.base_score, n * sizeof(double)));
    cc.out.hit = static_cast<uint8_t*>(out(cc.want.hit, n));
}

// The stage on a snapshot, products and start feet, with the outputs check_call_layout placed
void check_stage_fill(CheckCall& cc, const CallPlan& cp, const fpe_foothold* nominal, const uint8_t* cycleOk, const double* startFeet) {
    cc.stage.m = dev_map(*cp.snap);
    cc.stage.bm = cc.planes.bits;
    fpe::CheckArgs& a = cc.stage.a;
    a.nominal = nominal, a.cycleOk = cycleOk, a.startFeet = startFeet;
    a.swing = cc.out.swing, a.trunk = cc.out.trunk, a.margin = cc.out.margin, a.baseScore = cc.out.base_score, a.hit = cc.out.hit;
}

const fpe::CheckStage* check_call_stage(CheckCall& cc, const CallPlan& cp, const RankLayout& L) {
    // no check enabled: the score, the classes and the keys are the summary's; only base_score and hit would be left to write
    if (cc.stage.a.checks == 0 && !cc.out.base_score && !cc.out.hit) return nullptr;
    check_stage_fill(cc, cp, L.full.nominal, L.full.cycle_ok, L.full.stance);
    return &cc.stage;
}
}  // namespace

int fpe_check_plan_device(fpe_handle h, const fpe_params* params, const fpe_check_params* checks, const fpe_plan_out* d_products,
                          const double* d_start_feet, int32_t B, int32_t n_cycles, const fpe_check_out* d_out, void* stream) {
    if (!d_products || !d_out || !d_products->nominal) return fail(FPE_E_INVALID_ARG, "null argument");
    CheckCall cc;
    int rc = check_swing_shape(B, n_cycles);
    if (rc == FPE_OK) rc = check_check_args(params, checks, d_out, cc);
    if (rc != FPE_OK) return rc;
    const uint32_t on = cc.stage.a.checks;
    if (on == 0) return fail(FPE_E_INVALID_ARG, "no check enabled");
    if (d_out->base_score) return fail(FPE_E_INVALID_ARG, "the check stage alone computes no score: base_score must be NULL");
    if (!cc.want.swing && !cc.want.trunk && !cc.want.margin && !cc.want.hit)
        return fail(FPE_E_INVALID_ARG, "no output of an enabled check requested");
    if ((on & (FPE_CHECK_SWING | FPE_CHECK_TRUNK)) && !d_products->cycle_ok) return fail(FPE_E_INVALID_ARG, "null argument (cycle_ok)");
    if ((on & FPE_CHECK_SWING) && !d_start_feet && !d_products->stance)
        return fail(FPE_E_INVALID_ARG, "neither start feet nor the stance product given");
    hipStream_t st = static_cast<hipStream_t>(stream);
    CallPlan cp;
    rc = prepare_call(h, params, 0.0f, cp, st, false);
    if (rc == FPE_OK) rc = check_call_map(cc, cp);
    if (rc == FPE_OK) rc = check_call_planes(cc, *params, cp, st);
    if (rc != FPE_OK) return rc;
    mark_async_launch(cp);
    check_call_mark_async(cc);
    ArenaCursor none;
    check_call_layout(cc, none, B, false);
    check_stage_fill(cc, cp, d_products->nominal, d_products->cycle_ok, d_start_feet ? d_start_feet : d_products->stance);
    FPE_HIP(fpe::launch_plan_check(cc.stage, B, n_cycles, false, st));
    return FPE_OK;
}

int fpe_plan_rank_checked_device(fpe_handle h, const fpe_params* params, const fpe_rank_params* rank, const fpe_check_params* checks,
                                 const fpe_pose* d_poses, const fpe_stride* d_strides, int32_t B, int32_t n_cycles, int32_t K,
                                 const fpe_plan_out* d_full, const fpe_rank_out* d_out, const fpe_check_out* d_check_out, void* stream) {
    CheckCall cc;
    const int rc = check_check_args(params, checks, d_check_out, cc);
    if (rc != FPE_OK) return rc;
    return rank_device_call(h, params, rank, &cc, d_poses, d_strides, B, n_cycles, K, d_full, d_out, stream);
}

int fpe_plan_rank_checked(fpe_handle h, const fpe_params* params, const fpe_rank_params* rank, const fpe_check_params* checks,
                          const fpe_pose* poses, const fpe_stride* strides, int32_t B, int32_t n_cycles, int32_t K,
                          const fpe_rank_out* out, const fpe_check_out* check_out) {
    CheckCall cc;
    const int rc = check_check_args(params, checks, check_out, cc);
    if (rc != FPE_OK) return rc;
    return rank_host_call(h, params, rank, &cc, poses, strides, B, n_cycles, K, out);
}

// ---- checked beam (fpe_plan_beam_checked*; kernels: fpe_beam_check.hpp) ---------------------------------------------------------
namespace {
// The check stage of one beam call: the checked ranking's (its fpe_check_out is not used: a beam's check outputs are per slot),
// what the caller asked for, where the kernels write it, and the roots' start feet as the device sees them (null: the stance).
struct BeamCheckCall {
    CheckCall cc;
    fpe_beam_check_out want{};  // the caller's arrays (null: not wanted; those of a disabled check: cleared)
    fpe_beam_check_out out{};
    const double* dStartFeet = nullptr;
    bool haveStateIn = false;
    int waves = 1;  // wavefronts per candidate of beam_check_kernel (beam_check_map)
};

// Arguments of a checked beam's check stage that need no map: check_check_args' rules, and the start feet a swing needs
int check_beam_check_args(const fpe_params* params, const fpe_check_params* checks, const fpe_beam_check_out* out, bool haveStateIn,
                          const double* startFeet, BeamCheckCall& bc) {
    const int rc = check_check_args(params, checks, nullptr, bc.cc);
    if (rc != FPE_OK) return rc;
    const uint32_t on = bc.cc.stage.a.checks;
    if ((on & FPE_CHECK_SWING) && haveStateIn && !startFeet)
        return fail(FPE_E_INVALID_ARG, "a swing check of a beam from state_in needs start_feet: the state carries no z");
    if (out) bc.want = *out;
    if (!(on & FPE_CHECK_SWING)) bc.want.swing = nullptr;
    if (!(on & FPE_CHECK_TRUNK)) bc.want.trunk = nullptr;
    if (!(on & FPE_CHECK_MARGIN)) bc.want.margin = nullptr;
    bc.dStartFeet = startFeet;
    bc.haveStateIn = haveStateIn;
    return FPE_OK;
}

// One wavefront per candidate keeps every SIMD busy where a record covers few cells; where it covers thousands, the three checks one
// behind the other in one wavefront are the long pole and plan_check_kernel's four wavefronts per candidate win (measured at 198
// and at 3 080 cells under the body box: DESIGN.md 4.21).  The cells under the body box stand for the size of every record.
int beam_check_map(fpe_engine* h, BeamCheckCall& bc, const fpe_params& params, const CallPlan& cp) {
    int32_t knob;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        knob = h->tuning.beamCheckWaves;
    }
    const double res = cp.snap->g.res;
    const double boxCells = (static_cast<double>(params.length) / res) * (static_cast<double>(params.width) / res);
    bc.waves = knob ? knob : (boxCells > 1024.0 ? 4 : 1);
    return check_call_map(bc.cc, cp);
}
int beam_check_planes(BeamCheckCall& bc, const fpe_params& params, const CallPlan& cp, hipStream_t stream) {
    return check_call_planes(bc.cc, params, cp, stream);
}
void beam_check_mark_async(const BeamCheckCall& bc) { check_call_mark_async(bc.cc); }
bool beam_check_wants_stance(const BeamCheckCall& bc, bool haveStateIn) { return !bc.dStartFeet && !haveStateIn; }
void beam_check_set_start_feet(BeamCheckCall& bc, const double* d_startFeet) { bc.dStartFeet = d_startFeet; }
int beam_check_host_feet(const BeamCheckCall& bc, const double* startFeet, int32_t B) {
    if (!(bc.cc.stage.a.checks & FPE_CHECK_SWING) || !startFeet) return FPE_OK;  // (without the swing they only pass through to `feet`)
    for (int64_t q = 0; q < static_cast<int64_t>(B) * 4; ++q)
        if (!swing_point_ok(startFeet + q * 3)) return fail(FPE_E_INVALID_ARG, "start feet must be finite and within 1e6 m");
    return FPE_OK;
}

void beam_check_layout(BeamCheckCall& bc, BeamLayout& L, ArenaCursor& A, bool hostForm) {
    const fpe::BeamShape& sh = L.sh;
    const size_t slots_ = static_cast<size_t>(sh.B) * sh.slotStride, outSlots = static_cast<size_t>(sh.B) * sh.outStride;
    const size_t chains = static_cast<size_t>(sh.B) * (sh.S > 1 ? fpe::beam_live(sh, sh.S - 2) : 1) * sh.M;
    L.sc.candCheck = A.take(chains * fpe::kBeamCheckStateBytes);
    L.sc.parentsCheck = A.take(slots_ * fpe::kBeamCheckStateBytes);
    const auto out = [&](void* dst, size_t bytesPerSlot) {
        if (!dst || !hostForm) return dst;
        L.outSlot[A.outs.n] = bytesPerSlot;
        return A.out(dst, bytesPerSlot * outSlots);
    };
    bc.out.swing = static_cast<fpe_swing_summary*>(out(bc.want.swing, sizeof(fpe_swing_summary)));
    bc.out.trunk = static_cast<fpe_trunk_summary*>(out(bc.want.trunk, sizeof(fpe_trunk_summary)));
    bc.out.margin = static_cast<fpe_margin_summary*>(out(bc.want.margin, sizeof(fpe_margin_summary)));
    bc.out.base_penalty = static_cast<double*>(out(bc.want.base_penalty, sizeof(double)));
    bc.out.hit = static_cast<uint8_t*>(out(bc.want.hit, 1));
    bc.out.feet = static_cast<double*>(out(bc.want.feet, 12 * sizeof(double)));
}

int beam_check_prune(BeamCheckCall& bc, const CallPlan& cp, const fpe::BeamConsts& consts, const BeamLayout& L, int s, hipStream_t stream) {
    bc.cc.stage.m = dev_map(*cp.snap);
    bc.cc.stage.bm = bc.cc.planes.bits;
    fpe::BeamCheckArgs args{};
    args.bc = consts;
    if (bc.dStartFeet) args.rootFeet = bc.dStartFeet, args.rootFeetStride = 12;
    else if (!bc.haveStateIn) args.rootFeet = L.sc.cand.stance, args.rootFeetStride = 12 * L.sh.M;  // chain b * M: option 0's, as every option's
    FPE_HIP(fpe::launch_beam_prune_checked(L.sh, s, L.sc, bc.cc.stage, args, bc.waves, stream));
    return FPE_OK;
}

int beam_check_trace(BeamCheckCall& bc, const BeamLayout& L, hipStream_t stream) {
    FPE_HIP(fpe::launch_beam_trace_checked(L.sh, L.sc, L.out, bc.cc.stage.a.checks, bc.out, stream));
    return FPE_OK;
}
}  // namespace

int fpe_plan_beam_checked_device(fpe_handle h, const fpe_params* params, const fpe_beam_params* beam, const fpe_check_params* checks,
                                 const fpe_pose* d_poses, const fpe_plan_state* d_state_in, const double* d_start_feet, int32_t B,
                                 const fpe_stride* d_options, int32_t M, const fpe_beam_out* d_out,
                                 const fpe_beam_check_out* d_check_out, void* stream) {
    BeamCheckCall bc;
    const int rc = check_beam_check_args(params, checks, d_check_out, d_state_in != nullptr, d_start_feet, bc);
    if (rc != FPE_OK) return rc;
    // no check enabled: the unchecked beam's launches, check_out not touched
    return beam_device_call(h, params, beam, bc.cc.stage.a.checks ? &bc : nullptr, d_poses, d_state_in, B, d_options, M, d_out, stream);
}

int fpe_plan_beam_checked(fpe_handle h, const fpe_params* params, const fpe_beam_params* beam, const fpe_check_params* checks,
                          const fpe_pose* poses, const fpe_plan_state* state_in, const double* start_feet, int32_t B,
                          const fpe_stride* options, int32_t M, const fpe_beam_out* out, const fpe_beam_check_out* check_out) {
    BeamCheckCall bc;
    const int rc = check_beam_check_args(params, checks, check_out, state_in != nullptr, start_feet, bc);
    if (rc != FPE_OK) return rc;
    const uint32_t on = bc.cc.stage.a.checks;
    return beam_host_call(h, params, beam, on ? &bc : nullptr, poses, state_in, on ? start_feet : nullptr, B, options, M, out);
}

int fpe_last_service_gate(fpe_handle h, fpe_service_gate* out) {
    if (!h || !out) return fail(FPE_E_INVALID_ARG, "null argument");
    if (g_gateEngine != h) return fail(FPE_E_INVALID_ARG, "no fpe_plan_service* call was made with this engine on this thread");
    *out = g_gate;
    return FPE_OK;
}

int fpe_plan_service(fpe_handle h, const fpe_params* params, const double initial_position[3], uint8_t gait_cycles,
                     fpe_global_footholds* response) {
    return fpe_plan_service_ex(h, params, initial_position, gait_cycles, response, nullptr, nullptr, nullptr);
}

int fpe_plan_service_ex(fpe_handle h, const fpe_params* params, const double initial_position[3], uint8_t gait_cycles,
                        fpe_global_footholds* response, fpe_global_footholds* centroid, double* default_footholds,
                        int32_t* n_default_rows) {
    return fpe_plan_service_report(h, params, initial_position, gait_cycles, response, centroid, default_footholds,
                                   n_default_rows, nullptr, nullptr);
}

int fpe_plan_service_report(fpe_handle h, const fpe_params* params, const double initial_position[3], uint8_t gait_cycles,
                            fpe_global_footholds* response, fpe_global_footholds* centroid, double* default_footholds,
                            int32_t* n_default_rows, fpe_track_report* nominal_report, fpe_track_report* centroid_report) {
    return fpe_plan_service_opt(h, params, nullptr, initial_position, gait_cycles, response, centroid, default_footholds, n_default_rows,
                                nominal_report, centroid_report, nullptr, nullptr, nullptr);
}

int fpe_plan_service_opt(fpe_handle h, const fpe_params* params, const fpe_opt_params* opt, const double initial_position[3],
                         uint8_t gait_cycles, fpe_global_footholds* response, fpe_global_footholds* centroid,
                         double* default_footholds, int32_t* n_default_rows, fpe_track_report* nominal_report,
                         fpe_track_report* centroid_report, fpe_global_footholds* opt_msg, fpe_track_report* opt_report,
                         fpe_opt_cycle* opt_cycles) {
    g_gate = fpe_service_gate{255, FPE_GATE_NONE, 0, 0, {0, 0, 0, 0}, 0.0, 0.0};
    g_gateEngine = h;
    if (!initial_position || !response) return fail(FPE_E_INVALID_ARG, "null argument");
    if (default_footholds && !n_default_rows) return fail(FPE_E_INVALID_ARG, "n_default_rows is required with default_footholds");
    fpe_pose pose;
    std::memset(&pose, 0, sizeof(pose));
    pose.position[0] = initial_position[0];
    pose.position[1] = initial_position[1];
    pose.position[2] = initial_position[2];
    const int N = gait_cycles;
    double stance[12];
    std::vector<fpe_foothold> nominal(static_cast<size_t>(N) * 4);
    std::vector<fpe_centroid_foothold> cen(static_cast<size_t>(N) * 4);
    std::vector<fpe_opt_foothold> optf(static_cast<size_t>(N) * 4);
    std::vector<double> dflt(static_cast<size_t>(N) * 12);
    std::vector<uint8_t> ok(static_cast<size_t>(N));
    if (N == 0) {
        // the reference's loop body never runs (cpp:762); the stance comes from initialize()
        if (!h || !params) return fail(FPE_E_INVALID_ARG, "null handle or params");
        fpe::PlanConsts pc;
        fpe::derive_constants(*params, fpe::make_geom(1, 1, 1.0, 0.0, 0.0), params->searchRadius, fpe::Tuning(), pc);
        for (int l = 0; l < 4; ++l) {
            double sx = (l == 0 || l == 3) ? pc.LbHalf : -pc.LbHalf;
            double sy = (l <= 1) ? pc.WbHalfNeg : pc.WbHalfPos;
            double sz = 0;
            sx += pose.position[0];
            sy += pose.position[1];
            sz += pose.position[2];
            stance[l * 3] = sx; stance[l * 3 + 1] = sy; stance[l * 3 + 2] = sz;
        }
    } else {
        fpe_plan_out out;
        std::memset(&out, 0, sizeof(out));
        out.nominal = nominal.data();
        out.cycle_ok = ok.data();
        out.stance = stance;
        if (centroid || centroid_report) out.centroid = cen.data();
        if (default_footholds) out.default_next = dflt.data();
        // The handler's gate (cpp:920-934; include/fpe.h "service-shaped call"): cycle 0 by the plan kernels, the y side of
        // every cycle here on the host, the x side of cycles >= 1 by the opt track's chain — build-defined, run only when
        // an opt product is asked for or fpe_set_tuning("service_opt_gate", 1 | 2) wants its verdict.
        fpe_opt_out oout;
        std::memset(&oout, 0, sizeof(oout));
        uint8_t gateFail = 255;
        oout.gate_fail_cycle = &gateFail;
        // (the track's records only when a product is made of them: a call that wants the gate's verdict alone spares the chain
        // its heights — getFootholdMeanHeight on the gait-cycle submap, an elevation round trip per cycle — and its stores)
        oout.footholds = (opt_msg || opt_report || centroid_report) ? optf.data() : nullptr;
        oout.cycles = opt_cycles;
        double rowsAfter[2] = {0.0, 0.0};
        oout.rows_after = rowsAfter;
        int optGate = 2;
        if (h) {
            std::lock_guard<std::mutex> lk(h->mu);
            optGate = h->tuning.serviceOptGate;
        }
        const bool wantOptProduct = opt_msg || opt_report || opt_cycles || centroid_report;
        const bool runChain = wantOptProduct || optGate != 0;
        uint8_t poseStatus = 0;
        out.pose_status = &poseStatus;
        GateGeom gg;
        bool optDropped = false;
        int rc = plan_host(h, params, opt, &pose, 1, N, &out, nullptr, runChain ? &oout : nullptr, &gg, wantOptProduct ? nullptr : &optDropped);
        if (rc != FPE_OK) return rc;
        // exact verdicts: the first cycle (stance feet), then the lateral side of every cycle
        int lateral = 255;
        {
            double adjY = 0.0;  // ajustedPose_[1], cpp:759
            for (int c = 0; c < N; ++c) {
                const double py = pose.position[1] + adjY;  // cpp:2329
                // (x at the map's centre: the x side of getSubmap passes there, what is left is the y side)
                const bool okY = std::fabs(py) <= 1e6 && std::fabs(gg.g.posX) <= 1e6 && fpe::submap_info(gg.g, gg.g.posX, py, gg.isosLen, gg.isosWid).ok;
                if (!okY) {
                    lateral = c;
                    break;
                }
                adjY += gg.drift;  // cpp:1578
            }
        }
        const bool chainRan = runChain && !optDropped;
        fpe_service_gate gate = g_gate;  // (reset at entry)
        gate.chain_ran = chainRan ? 1 : 0;
        gate.lf_current_row = chainRan ? rowsAfter[0] : 0.0;
        gate.rh_current_row = chainRan ? rowsAfter[1] : 0.0;
        auto verdict = [&](int cycle, int kind) {
            gate.fail_cycle = static_cast<uint8_t>(cycle);
            gate.fail_kind = static_cast<uint8_t>(kind);
        };
        if (poseStatus & FPE_POSE_OPT_SUBMAP_FAILED) verdict(0, FPE_GATE_CYCLE0);
        else if (lateral != 255) verdict(lateral, FPE_GATE_LATERAL);  // (exact kinds first: the reference refuses in cycle `lateral` at the latest)
        else if (chainRan && gateFail != 255) verdict(gateFail, gateFail == 0 ? FPE_GATE_CYCLE0 : FPE_GATE_BUILD_DEFINED);
        const bool refuse = gate.fail_kind == FPE_GATE_CYCLE0 || gate.fail_kind == FPE_GATE_LATERAL ||
                            (gate.fail_kind == FPE_GATE_BUILD_DEFINED && optGate == 2);
        gate.returned_false = refuse ? 1 : 0;
        g_gate = gate;
        if (refuse) {
            // getGaitCycleSearchGridMap fails in cycle gate.fail_cycle: the reference's handler logs "Failed to get gait-cycle
            // search gridmap." and returns false (cpp:931-934); the ROS response is never assigned (cpp:1588 is not reached)
            std::memset(response, 0, sizeof(*response));
            if (centroid) std::memset(centroid, 0, sizeof(*centroid));
            if (n_default_rows) *n_default_rows = 0;
            if (nominal_report) std::memset(nominal_report, 0, sizeof(*nominal_report));
            if (centroid_report) std::memset(centroid_report, 0, sizeof(*centroid_report));
            if (opt_msg) std::memset(opt_msg, 0, sizeof(*opt_msg));
            if (opt_report) std::memset(opt_report, 0, sizeof(*opt_report));
            static const char* const kinds[] = {"", "first gait cycle", "lateral side", "x side, build-defined optimiser"};
            return fail(FPE_E_SERVICE_FALSE, "getGaitCycleSearchGridMap: getSubmap failed in gait cycle " + std::to_string(static_cast<int>(gate.fail_cycle)) +
                                                 " (" + kinds[gate.fail_kind] + "; cpp:931-934)");
        }
    }
    // The call answers although the opt track's chain stopped at its gate (modes 0 / 1: the verdict is advisory): the chain's
    // products end where it stopped and the reference would not have published them — its handler returns false at that gate,
    // whatever its optimiser (cpp:931-934).  They are handed back EMPTY, never as the truncated track of an aborted chain; the
    // kind and cycle are in fpe_last_service_gate.
    const bool chainAborted = g_gate.chain_ran && g_gate.fail_kind == FPE_GATE_BUILD_DEFINED;
    fpe::assemble_global_footholds(nominal.data(), ok.data(), stance, N, response);
    if (centroid) fpe::assemble_centroid_footholds(cen.data(), ok.data(), stance, N, centroid);
    if (opt_msg) {
        if (chainAborted) std::memset(opt_msg, 0, sizeof(*opt_msg));
        else fpe::assemble_opt_footholds(optf.data(), ok.data(), stance, N, opt_msg);
    }
    if (nominal_report || centroid_report || opt_report) {
        if (!params) return fail(FPE_E_INVALID_ARG, "null params");
        std::vector<double> xyz(static_cast<size_t>(N) * 12);
        if (nominal_report) {
            for (size_t k = 0; k < static_cast<size_t>(N) * 4; ++k) {
                xyz[k * 3] = nominal[k].x;
                xyz[k * 3 + 1] = nominal[k].y;
                xyz[k * 3 + 2] = static_cast<double>(nominal[k].z);
            }
            fpe::assemble_track_report(xyz.data(), ok.data(), stance, N, *params, nominal_report);
        }
        if (centroid_report || opt_report) {
            std::unique_ptr<fpe_track_report> optRep(new (std::nothrow) fpe_track_report);
            if (!optRep) return fail(FPE_E_NOMEM, "out of host memory");
            for (size_t k = 0; k < static_cast<size_t>(N) * 4; ++k) {
                xyz[k * 3] = optf[k].x;
                xyz[k * 3 + 1] = optf[k].y;
                xyz[k * 3 + 2] = static_cast<double>(optf[k].z);
            }
            fpe::assemble_track_report(xyz.data(), ok.data(), stance, N, *params, optRep.get());
            if (chainAborted) std::memset(optRep.get(), 0, sizeof(fpe_track_report));  // (no opt path, no opt KPIs; the centroid path is then the centroid track's own)
            if (opt_report) std::memcpy(opt_report, optRep.get(), sizeof(*opt_report));
            if (centroid_report) {
                for (size_t k = 0; k < static_cast<size_t>(N) * 4; ++k) {
                    xyz[k * 3] = cen[k].x;
                    xyz[k * 3 + 1] = cen[k].y;
                    xyz[k * 3 + 2] = static_cast<double>(cen[k].z);
                }
                fpe::assemble_track_report(xyz.data(), ok.data(), stance, N, *params, centroid_report);
                if (!chainAborted) fpe::interleave_centroid_path(centroid_report, *optRep);  // cpp:946: the opt track pushes onto the same path
            }
        }
    }
    if (default_footholds) {
        int rows = 0;
        std::memcpy(default_footholds, stance, 12 * sizeof(double));  // cpp:666-671
        rows = 1;
        for (int g = 0; g < N; ++g)
            if (ok[g]) {  // cpp:1344-1348: appended only for committed cycles
                std::memcpy(default_footholds + static_cast<size_t>(rows) * 12, dflt.data() + static_cast<size_t>(g) * 12,
                            12 * sizeof(double));
                ++rows;
            }
        *n_default_rows = rows;
    }
    return FPE_OK;
}

}  // extern "C"

// ---- scan fusion (fpe_scan_*; include/fpe.h): the scan state, the fuse, and the way into the planner's snapshot ------------------
// A state owns two pairs of canonical layers (the current one and the one a move writes), the fuse's scratch (16 bytes per cell, at
// rest between calls), the accumulators of a call's info, the point records (grown on demand) and — for the host forms — a stream,
// a points staging buffer and a device info.  Ordering: `last` is recorded behind every operation on whatever stream it ran, and
// every operation waits for it GPU-side first (the filter scratch's pattern, filter_slot_take); `mu` makes the order in which the
// operations are queued the order of those events.
struct fpe_scan_state {
    fpe_engine* h = nullptr;
    std::mutex mu;
    fpe::MapGeom g;
    size_t n = 0;
    float* elev[2] = {nullptr, nullptr};  // [cur]: the layer; [cur ^ 1]: the second buffer (a move's destination, a host set's staging)
    float* var[2] = {nullptr, nullptr};
    int cur = 0;
    fpe::ScanCell* cells = nullptr;
    int32_t* acc = nullptr;  // kScanAccWords accumulators, then twice sixteen words: the host forms' device infos (the fuse's, the clear's)
    uint2* rec = nullptr;
    size_t recCap = 0;       // records
    float* pts = nullptr;    // the host forms' staging: points, or an image at its own size and its two tables (scan_stage)
    size_t ptsCap = 0;       // floats
    float* trav = nullptr;   // fpe_scan_install's traversability layer (allocated by the first install)
    float* closed = nullptr;     // the closed elevation the planner gets (fpe_scan_install_closed, fpe_scan_ingest_closed) and the host close's
                                 // staging; allocated by the first close, with:
    int32_t* closeAcc = nullptr; // the close's own accumulators and the host forms' device info (kCloseAccWords)
    bool closeFresh = false;     // closeAcc still has to be reset, on the stream of the first close
    hipEvent_t last = nullptr;
    hipStream_t own = nullptr;
};

namespace {

constexpr int kScanMergeDefault = 2;  // "scan_merge" 0: the form measured faster on both workloads of profiles/scan_summary.txt
// "scan_clear_form" / "scan_clear_group" 0: the form measured faster on the depth image of profiles/scan_clear_summary.txt
constexpr int kScanClearFormDefault = 1;
constexpr int kScanClearGroupDefault = 16;
constexpr int kScanCloseFormDefault = 2;  // "scan_close_form" 0: see profiles/scan_close_summary.txt

// An operation of a state on `stream`: behind the state's last one, and its own event recorded on every way out (an operation that
// failed half-way may have queued work the next one must not overtake).  The caller holds s->mu.
struct ScanOp {
    fpe_scan_state* s;
    hipStream_t stream;
    bool entered = false;
    int enter() {
        FPE_HIP(hipSetDevice(s->h->device));
        FPE_HIP(hipStreamWaitEvent(stream, s->last, 0));
        entered = true;
        return FPE_OK;
    }
    ~ScanOp() {
        if (entered) (void)hipEventRecord(s->last, stream);
    }
};

fpe_map_desc scan_desc(const fpe_scan_state* s) {
    fpe_map_desc d;
    std::memset(&d, 0, sizeof(d));
    d.rows = s->g.rows;
    d.cols = s->g.cols;
    d.resolution = s->g.res;
    d.position[0] = s->g.posX;
    d.position[1] = s->g.posY;
    d.storage_order = 1;
    return d;
}

template <class T>
int scan_grow(T*& buf, size_t& cap, size_t want) {
    if (want <= cap) return FPE_OK;
    T* p = nullptr;
    FPE_HIP(hipMalloc(reinterpret_cast<void**>(&p), want * sizeof(T)));
    if (buf) (void)hipFree(buf);  // (synchronises the device: nothing still reads the old buffer)
    buf = p;
    cap = want;
    return FPE_OK;
}

int scan_set_layers(fpe_scan_state* s, const float* elev, const float* var, bool onDevice, hipStream_t stream) {
    if (!s || !elev || !var) return fail(FPE_E_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    ScanOp op{s, onDevice ? stream : s->own};
    int rc = op.enter();
    if (rc != FPE_OK) return rc;
    const int c = s->cur;
    if (!onDevice) {  // staged in the second buffer pair
        FPE_HIP(hipMemcpyAsync(s->elev[c ^ 1], elev, s->n * sizeof(float), hipMemcpyHostToDevice, op.stream));
        FPE_HIP(hipMemcpyAsync(s->var[c ^ 1], var, s->n * sizeof(float), hipMemcpyHostToDevice, op.stream));
        elev = s->elev[c ^ 1];
        var = s->var[c ^ 1];
    }
    FPE_HIP(fpe::launch_scan_set(reinterpret_cast<const uint32_t*>(elev), reinterpret_cast<const uint32_t*>(var), reinterpret_cast<uint32_t*>(s->elev[c]),
                                 reinterpret_cast<uint32_t*>(s->var[c]), s->n, op.stream));
    if (!onDevice) FPE_HIP(hipStreamSynchronize(op.stream));
    return FPE_OK;
}

int scan_read_layers(fpe_scan_state* s, float* elev, float* var, bool onDevice, hipStream_t stream) {
    if (!s || (!elev && !var)) return fail(FPE_E_INVALID_ARG, "null state, or no layer requested");
    std::lock_guard<std::mutex> lk(s->mu);
    ScanOp op{s, onDevice ? stream : s->own};
    int rc = op.enter();
    if (rc != FPE_OK) return rc;
    const hipMemcpyKind kind = onDevice ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (elev) FPE_HIP(hipMemcpyAsync(elev, s->elev[s->cur], s->n * sizeof(float), kind, op.stream));
    if (var) FPE_HIP(hipMemcpyAsync(var, s->var[s->cur], s->n * sizeof(float), kind, op.stream));
    if (!onDevice) FPE_HIP(hipStreamSynchronize(op.stream));
    return FPE_OK;
}

// (the caller holds s->mu and has entered `stream`)
int scan_move_locked(fpe_scan_state* s, const int32_t shift[2], const double position[2], hipStream_t stream) {
    const int rows = s->g.rows, cols = s->g.cols, c = s->cur;
    const int sr = std::max(-rows, std::min(rows, shift[0])), sc = std::max(-cols, std::min(cols, shift[1]));  // beyond: nothing is carried either way
    FPE_HIP(fpe::launch_scan_move(reinterpret_cast<const uint32_t*>(s->elev[c]), reinterpret_cast<const uint32_t*>(s->var[c]),
                                  reinterpret_cast<uint32_t*>(s->elev[c ^ 1]), reinterpret_cast<uint32_t*>(s->var[c ^ 1]), rows, cols, sr, sc, stream));
    s->cur = c ^ 1;
    s->g = fpe::make_geom(rows, cols, s->g.res, position[0], position[1]);
    return FPE_OK;
}

// The point source of a fuse, a clear or an ingest: points with the scan's stride, or an image (its descriptor and its elements;
// point 6 of the scan block).  As the entry points take it the addresses are the caller's (host or device); scan_stage gives the
// device form of a host source; the *_locked routines take device addresses only.
struct ScanSource {
    bool isImage = false;
    const float* points = nullptr;
    const fpe_scan_image* im = nullptr;
    const void* image = nullptr;
    const float* rowDir = nullptr;  // the tables' addresses as the kernels read them (device forms: the descriptor's)
    const float* colDir = nullptr;
    static ScanSource of_points(const float* points) {
        ScanSource r;
        r.points = points;
        return r;
    }
    static ScanSource of_image(const fpe_scan_image* im, const void* image) {
        ScanSource r;
        r.isImage = true;
        r.im = im;
        r.image = image;
        if (im) {
            r.rowDir = im->row_dir;
            r.colDir = im->col_dir;
        }
        return r;
    }
    bool given() const { return isImage ? (im != nullptr && image != nullptr) : points != nullptr; }
};

// The three passes on `stream` (the caller holds s->mu, has validated the call and has entered `stream`).
int scan_fuse_locked(fpe_scan_state* s, const fpe_scan_params* sp, const fpe_scan* scan, const ScanSource& src, fpe_scan_info* d_info, hipStream_t stream) {
    int rc = scan_grow(s->rec, s->recCap, static_cast<size_t>(scan->n_points));
    if (rc != FPE_OK) return rc;
    int merge;
    {
        std::lock_guard<std::mutex> lk(s->h->mu);
        merge = s->h->tuning.scanMerge;
    }
    if (merge == 0) merge = kScanMergeDefault;
    fpe::ScanArgs a;
    fpe::scan_consts(*sp, *scan, s->g, a);
    a.points = src.points;
    a.rec = s->rec;
    a.cells = s->cells;
    a.acc = s->acc;
    a.elev = reinterpret_cast<uint32_t*>(s->elev[s->cur]);
    a.var = reinterpret_cast<uint32_t*>(s->var[s->cur]);
    a.info = reinterpret_cast<int32_t*>(d_info);
    if (src.isImage) {  // (one form of the top pass: "scan_merge" does not apply)
        fpe::scan_image_consts(*src.im, src.image, src.rowDir, src.colDir, a.im);
        FPE_HIP(fpe::launch_scan_fuse_image(a, stream));
    } else {
        FPE_HIP(fpe::launch_scan_fuse(a, merge == 2, stream));
    }
    return FPE_OK;
}

// The two passes of a clear on `stream` (the caller holds s->mu, has validated the call and has entered `stream`).
int scan_clear_locked(fpe_scan_state* s, const fpe_scan_params* sp, const fpe_scan_clear_params* cp, const fpe_scan* scan, const ScanSource& src,
                      fpe_scan_clear_info* d_info, hipStream_t stream) {
    int form, group;
    {
        std::lock_guard<std::mutex> lk(s->h->mu);
        form = s->h->tuning.scanClearForm;
        group = s->h->tuning.scanClearGroup;
    }
    if (form == 0) form = kScanClearFormDefault;
    if (group == 0) group = kScanClearGroupDefault;
    fpe::ScanClearArgs a;
    fpe::scan_clear_consts(*sp, *cp, *scan, s->g, a);
    a.points = src.points;
    a.cells = s->cells;
    a.acc = s->acc;
    a.elev = reinterpret_cast<uint32_t*>(s->elev[s->cur]);
    a.var = reinterpret_cast<uint32_t*>(s->var[s->cur]);
    a.info = reinterpret_cast<int32_t*>(d_info);
    if (src.isImage) {
        fpe::scan_image_consts(*src.im, src.image, src.rowDir, src.colDir, a.im);
        FPE_HIP(fpe::launch_scan_clear_image(a, form, group, stream));
    } else {
        FPE_HIP(fpe::launch_scan_clear(a, form, group, stream));
    }
    return FPE_OK;
}

// The close's buffers, allocated by a state's first close (the caller holds s->mu and has set the device); the accumulators are
// reset by scan_close_locked on the stream of that close, which every later operation of the state is ordered behind.
int scan_close_alloc(fpe_scan_state* s) {
    if (!s->closed) FPE_HIP(hipMalloc(reinterpret_cast<void**>(&s->closed), s->n * sizeof(float) + kLayerPadBytes));
    if (!s->closeAcc) {
        FPE_HIP(hipMalloc(reinterpret_cast<void**>(&s->closeAcc), fpe::kCloseAccWords * sizeof(int32_t)));
        s->closeFresh = true;
    }
    return FPE_OK;
}

// The one launch of a close on `stream` (the caller holds s->mu, has validated the call, has called scan_close_alloc and has entered
// `stream`).  The state's layers and scratch are only read.
int scan_close_locked(fpe_scan_state* s, const fpe_scan_close_params* kp, const int32_t rect[4], float* d_out, int64_t outStride, uint8_t* d_cls,
                      fpe_scan_close_info* d_info, hipStream_t stream) {
    int form;
    {
        std::lock_guard<std::mutex> lk(s->h->mu);
        form = s->h->tuning.scanCloseForm;
    }
    if (form == 0) form = kScanCloseFormDefault;
    if (s->closeFresh) {
        FPE_HIP(fpe::launch_scan_close_reset(s->closeAcc, stream));
        s->closeFresh = false;
    }
    fpe::ScanCloseArgs a;
    fpe::scan_close_consts(*kp, rect, s->g.rows, s->g.cols, a);
    a.outStride = outStride;
    a.elev = reinterpret_cast<const uint32_t*>(s->elev[s->cur]);
    a.out = reinterpret_cast<uint32_t*>(d_out);
    a.cls = d_cls;
    a.acc = s->closeAcc;
    a.info = reinterpret_cast<int32_t*>(d_info);
    FPE_HIP(fpe::launch_scan_close(a, form, stream));
    return FPE_OK;
}

int scan_close_check(const fpe_scan_state* s, const fpe_scan_close_params* kp, const int32_t rect[4]) {
    const char* why = "";
    const int rc = fpe::check_scan_close(s->g.rows, s->g.cols, kp, rect, &why);
    return rc == FPE_OK ? rc : fail(rc, why);
}

// The rectangles an ingest closes (include/fpe.h): the roi grown by the reach, then the strips whose neighbours a move took off the map.
int scan_close_rects(const fpe_scan_state* s, const fpe_scan_close_params* kp, const fpe_scan* scan, const int32_t shift[2], int32_t rects[3][4]) {
    const int rows = s->g.rows, cols = s->g.cols, R = kp->reach;
    const int r0 = std::max(0, scan->roi[0] - R), c0 = std::max(0, scan->roi[1] - R);
    const int r1 = std::min<int64_t>(rows, static_cast<int64_t>(scan->roi[0]) + scan->roi[2] + R);
    const int c1 = std::min<int64_t>(cols, static_cast<int64_t>(scan->roi[1]) + scan->roi[3] + R);
    int n = 0;
    const auto put = [&](int a, int b, int c, int d) {
        rects[n][0] = a, rects[n][1] = b, rects[n][2] = c, rects[n][3] = d;
        ++n;
    };
    put(r0, c0, r1 - r0, c1 - c0);
    if (shift[0] != 0) put(shift[0] > 0 ? 0 : rows - R, 0, R, cols);
    if (shift[1] != 0) put(0, shift[1] > 0 ? 0 : cols - R, rows, R);
    return n;
}

int scan_close_common(fpe_scan_state* s, const fpe_scan_close_params* kp, const int32_t rect[4], float* out, int64_t outStride, uint8_t* cls,
                      fpe_scan_close_info* info, bool onDevice, hipStream_t stream) {
    if (!s || !out) return fail(FPE_E_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    int rc = scan_close_check(s, kp, rect);
    if (rc != FPE_OK) return rc;
    if (outStride < rect[3]) return fail(FPE_E_INVALID_ARG, "out_row_stride below the rectangle's columns");
    FPE_HIP(hipSetDevice(s->h->device));
    rc = scan_close_alloc(s);
    if (rc != FPE_OK) return rc;
    ScanOp op{s, onDevice ? stream : s->own};
    rc = op.enter();
    if (rc != FPE_OK) return rc;
    if (onDevice) return scan_close_locked(s, kp, rect, out, outStride, cls, info, stream);
    // host form: the rectangle is closed into `closed` (dense), the classes into the second elevation buffer (a staging area, as for
    // a host set), and both come back with their pitch
    const size_t nr = static_cast<size_t>(rect[2]), nc = static_cast<size_t>(rect[3]);
    uint8_t* dCls = cls ? reinterpret_cast<uint8_t*>(s->elev[s->cur ^ 1]) : nullptr;
    fpe_scan_close_info* dInfo = reinterpret_cast<fpe_scan_close_info*>(s->closeAcc + fpe::kCloseAccInfo);
    rc = scan_close_locked(s, kp, rect, s->closed, rect[3], dCls, dInfo, s->own);
    if (rc != FPE_OK) return rc;
    fpe_scan_close_info got;
    FPE_HIP(hipMemcpy2DAsync(out, static_cast<size_t>(outStride) * sizeof(float), s->closed, nc * sizeof(float), nc * sizeof(float), nr, hipMemcpyDeviceToHost,
                             s->own));
    if (cls) FPE_HIP(hipMemcpy2DAsync(cls, static_cast<size_t>(outStride), dCls, nc, nc, nr, hipMemcpyDeviceToHost, s->own));
    FPE_HIP(hipMemcpyAsync(&got, dInfo, sizeof(got), hipMemcpyDeviceToHost, s->own));
    FPE_HIP(hipStreamSynchronize(s->own));
    if (info) *info = got;
    return FPE_OK;
}

// (cp == nullptr with withClear == false: the fuse's refusals alone; an image source: then the descriptor's and n_points against it)
int scan_check(const fpe_scan_state* s, const fpe_scan_params* sp, const fpe_scan_clear_params* cp, bool withClear, const fpe_scan* scan,
               const ScanSource& src) {
    const char* why = "";
    int rc = withClear ? fpe::check_scan_clear(s->g.rows, s->g.cols, sp, cp, scan, &why) : fpe::check_scan(s->g.rows, s->g.cols, sp, scan, &why);
    if (rc == FPE_OK && src.isImage) rc = fpe::check_scan_image(s->g.rows, s->g.cols, sp, nullptr, scan, src.im, &why);
    return rc == FPE_OK ? rc : fail(rc, why);
}

// A host source into the state's staging buffer on its own stream (entered); `dev` is its device form.  Points: n_points *
// point_stride floats.  An image at its own size: the elements up to the last pixel of the last row, then (spherical) the two tables.
int scan_stage(fpe_scan_state* s, const fpe_scan* scan, const ScanSource& src, ScanSource& dev) {
    dev = src;
    if (!src.isImage) {
        const size_t nf = static_cast<size_t>(scan->n_points) * static_cast<size_t>(scan->point_stride);
        const int rc = scan_grow(s->pts, s->ptsCap, std::max<size_t>(nf, 3));
        if (rc != FPE_OK) return rc;
        if (nf) FPE_HIP(hipMemcpyAsync(s->pts, src.points, nf * sizeof(float), hipMemcpyHostToDevice, s->own));
        dev.points = s->pts;
        return FPE_OK;
    }
    const fpe_scan_image& im = *src.im;
    const size_t elems = static_cast<size_t>(im.height - 1) * static_cast<size_t>(im.row_pitch) + static_cast<size_t>(im.width);
    const size_t bytes = elems * (im.format == FPE_SCAN_DEPTH_U16 ? 2 : 4);
    const size_t imageFloats = (bytes + 3) / 4;
    const bool tables = im.model == FPE_SCAN_IMAGE_SPHERICAL;
    const size_t rowFloats = tables ? 2 * static_cast<size_t>(im.height) : 0, colFloats = tables ? 2 * static_cast<size_t>(im.width) : 0;
    const int rc = scan_grow(s->pts, s->ptsCap, imageFloats + rowFloats + colFloats);
    if (rc != FPE_OK) return rc;
    FPE_HIP(hipMemcpyAsync(s->pts, src.image, bytes, hipMemcpyHostToDevice, s->own));
    dev.image = s->pts;
    dev.rowDir = dev.colDir = nullptr;
    if (tables) {
        FPE_HIP(hipMemcpyAsync(s->pts + imageFloats, im.row_dir, rowFloats * sizeof(float), hipMemcpyHostToDevice, s->own));
        FPE_HIP(hipMemcpyAsync(s->pts + imageFloats + rowFloats, im.col_dir, colFloats * sizeof(float), hipMemcpyHostToDevice, s->own));
        dev.rowDir = s->pts + imageFloats;
        dev.colDir = s->pts + imageFloats + rowFloats;
    }
    return FPE_OK;
}

int scan_fuse_common(fpe_scan_state* s, const fpe_scan_params* sp, const fpe_scan* scan, const ScanSource& src, fpe_scan_info* info, bool onDevice,
                     hipStream_t stream) {
    if (!s || !src.given()) return fail(FPE_E_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    int rc = scan_check(s, sp, nullptr, false, scan, src);
    if (rc != FPE_OK) return rc;
    ScanOp op{s, onDevice ? stream : s->own};
    rc = op.enter();
    if (rc != FPE_OK) return rc;
    if (onDevice) return scan_fuse_locked(s, sp, scan, src, info, stream);
    ScanSource dev;
    rc = scan_stage(s, scan, src, dev);
    if (rc != FPE_OK) return rc;
    fpe_scan_info* dInfo = reinterpret_cast<fpe_scan_info*>(s->acc + fpe::kScanAccWords);
    rc = scan_fuse_locked(s, sp, scan, dev, dInfo, s->own);
    if (rc != FPE_OK) return rc;
    fpe_scan_info got;
    FPE_HIP(hipMemcpyAsync(&got, dInfo, sizeof(got), hipMemcpyDeviceToHost, s->own));
    FPE_HIP(hipStreamSynchronize(s->own));
    if (info) *info = got;
    return FPE_OK;
}

int scan_clear_common(fpe_scan_state* s, const fpe_scan_params* sp, const fpe_scan_clear_params* cp, const fpe_scan* scan, const ScanSource& src,
                      fpe_scan_clear_info* info, bool onDevice, hipStream_t stream) {
    if (!s || !src.given()) return fail(FPE_E_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    int rc = scan_check(s, sp, cp, true, scan, src);
    if (rc != FPE_OK) return rc;
    ScanOp op{s, onDevice ? stream : s->own};
    rc = op.enter();
    if (rc != FPE_OK) return rc;
    if (onDevice) return scan_clear_locked(s, sp, cp, scan, src, info, stream);
    ScanSource dev;
    rc = scan_stage(s, scan, src, dev);
    if (rc != FPE_OK) return rc;
    fpe_scan_clear_info* dInfo = reinterpret_cast<fpe_scan_clear_info*>(s->acc + fpe::kScanAccWords + 16);
    rc = scan_clear_locked(s, sp, cp, scan, dev, dInfo, s->own);
    if (rc != FPE_OK) return rc;
    fpe_scan_clear_info got;
    FPE_HIP(hipMemcpyAsync(&got, dInfo, sizeof(got), hipMemcpyDeviceToHost, s->own));
    FPE_HIP(hipStreamSynchronize(s->own));
    if (info) *info = got;
    return FPE_OK;
}

// fpe_scan_ingest* (withClear false: cp and clearInfo unused), fpe_scan_ingest_clear* (the clear between the move and the fuse) and
// fpe_scan_ingest_closed* (withClose: behind the fuse the close of up to three rectangles into `closed`, which the patches then carry
// in place of the state's own elevation; withClose false: kp and closeInfo unused); fpe_scan_ingest_image* is all three, by its cp and kp
int scan_ingest_common(fpe_engine* h, fpe_scan_state* s, const fpe_filter_params* fp, const fpe_scan_params* sp, const fpe_scan_clear_params* cp,
                       bool withClear, const fpe_scan_close_params* kp, bool withClose, const fpe_scan* scan, const ScanSource& given, const int32_t shift[2],
                       const double position[2], fpe_scan_clear_info* clearInfo, fpe_scan_info* scanInfo, fpe_scan_close_info* closeInfo,
                       fpe_elevation_update_info* updateInfo, bool onDevice, hipStream_t stream) {
    if (!h || !s || !given.given() || !shift || !position) return fail(FPE_E_INVALID_ARG, "null argument");
    if (s->h != h) return fail(FPE_E_INVALID_ARG, "the scan state belongs to another engine");
    std::lock_guard<std::mutex> lk(s->mu);
    // every refusal ahead of the first queued operation
    int rc = scan_check(s, sp, cp, withClear, scan, given);
    if (rc != FPE_OK) return rc;
    int32_t rects[3][4];
    int nRects = 0;
    if (withClose) {
        if (!kp) return fail(FPE_E_INVALID_ARG, "null close parameters");
        const int32_t whole[4] = {0, 0, s->g.rows, s->g.cols};
        rc = scan_close_check(s, kp, whole);  // (the parameters; the rectangles below lie inside by construction)
        if (rc != FPE_OK) return rc;
        nRects = scan_close_rects(s, kp, scan, shift, rects);
        FPE_HIP(hipSetDevice(h->device));
        rc = scan_close_alloc(s);  // (the patches below point into `closed`)
        if (rc != FPE_OK) return rc;
    }
    fpe_map_update u;
    std::memset(&u, 0, sizeof(u));
    u.shift[0] = shift[0];
    u.shift[1] = shift[1];
    u.position[0] = position[0];
    u.position[1] = position[1];
    u.n_patches = 1;
    auto patch = [&]() {  // scan->roi of the state's CURRENT elevation layer, row-major with the layer's pitch; or the closed rectangles
        const float* e = s->elev[s->cur] + static_cast<size_t>(scan->roi[0]) * s->g.cols + scan->roi[1];
        u.patch[0] = fpe_map_patch{scan->roi[0], scan->roi[1], scan->roi[2], scan->roi[3], nullptr, e, s->g.cols, 1};
        for (int k = 0; k < nRects; ++k) {
            const int32_t* r = rects[k];
            u.patch[k] = fpe_map_patch{r[0], r[1], r[2], r[3], nullptr, s->closed + static_cast<size_t>(r[0]) * s->g.cols + r[1], s->g.cols, 1};
        }
        if (nRects) u.n_patches = nRects;
    };
    patch();
    {
        std::shared_ptr<MapSnapshot> snap;
        {
            std::lock_guard<std::mutex> lkE(h->mu);
            snap = h->map;
        }
        if (!snap) return fail(FPE_E_NO_MAP, "no map uploaded");
        if (snap->g.rows != s->g.rows || snap->g.cols != s->g.cols || snap->g.res != s->g.res)
            return fail(FPE_E_INVALID_ARG, "the snapshot's size or resolution differs from the scan state's");
        fpe::ElevationUpdatePlan plan;
        const char* why = "";
        rc = fpe::plan_elevation_update(s->g.rows, s->g.cols, s->g.res, fp, &u, plan, &why);
        if (rc != FPE_OK) return fail(rc, why);
    }
    ScanOp op{s, onDevice ? stream : s->own};
    rc = op.enter();
    if (rc != FPE_OK) return rc;
    fpe_scan_info* dInfo = scanInfo;
    fpe_scan_clear_info* dClearInfo = clearInfo;
    fpe_scan_close_info* dCloseInfo = closeInfo;
    ScanSource src = given;
    if (!onDevice) {
        rc = scan_stage(s, scan, given, src);
        if (rc != FPE_OK) return rc;
        dInfo = reinterpret_cast<fpe_scan_info*>(s->acc + fpe::kScanAccWords);
        dClearInfo = reinterpret_cast<fpe_scan_clear_info*>(s->acc + fpe::kScanAccWords + 16);
        if (withClose) dCloseInfo = reinterpret_cast<fpe_scan_close_info*>(s->closeAcc + fpe::kCloseAccInfo);
    }
    if (shift[0] != 0 || shift[1] != 0 || position[0] != s->g.posX || position[1] != s->g.posY) {
        rc = scan_move_locked(s, shift, position, op.stream);
        if (rc != FPE_OK) return rc;
        patch();  // (the move swapped the buffers)
    }
    if (withClear) {
        rc = scan_clear_locked(s, sp, cp, scan, src, dClearInfo, op.stream);
        if (rc != FPE_OK) return rc;
    }
    rc = scan_fuse_locked(s, sp, scan, src, dInfo, op.stream);
    if (rc != FPE_OK) return rc;
    for (int k = 0; k < nRects; ++k) {  // (close_info describes the first rectangle; the strips write none)
        const int32_t* r = rects[k];
        rc = scan_close_locked(s, kp, r, s->closed + static_cast<size_t>(r[0]) * s->g.cols + r[1], s->g.cols, nullptr, k == 0 ? dCloseInfo : nullptr, op.stream);
        if (rc != FPE_OK) return rc;
    }
    rc = update_elevation_common(h, fp, &u, updateInfo, true, op.stream);
    if (rc != FPE_OK) return rc;
    if (!onDevice) {
        fpe_scan_info got;
        fpe_scan_clear_info gotClear;
        fpe_scan_close_info gotClose;
        FPE_HIP(hipMemcpyAsync(&got, dInfo, sizeof(got), hipMemcpyDeviceToHost, op.stream));
        if (withClose) FPE_HIP(hipMemcpyAsync(&gotClose, dCloseInfo, sizeof(gotClose), hipMemcpyDeviceToHost, op.stream));
        if (withClear) FPE_HIP(hipMemcpyAsync(&gotClear, dClearInfo, sizeof(gotClear), hipMemcpyDeviceToHost, op.stream));
        FPE_HIP(hipStreamSynchronize(op.stream));
        if (scanInfo) *scanInfo = got;
        if (withClear && clearInfo) *clearInfo = gotClear;
        if (withClose && closeInfo) *closeInfo = gotClose;
    }
    return FPE_OK;
}

}  // namespace

extern "C" {

int fpe_scan_create(fpe_handle h, const fpe_map_desc* geom, fpe_scan_handle* out) {
    if (!out) return fail(FPE_E_INVALID_ARG, "null out handle");
    *out = nullptr;
    if (!h) return fail(FPE_E_INVALID_ARG, "null handle");
    int rc = check_desc(geom);
    if (rc != FPE_OK) return rc;
    if (geom->start_index[0] != 0 || geom->start_index[1] != 0 || geom->storage_order != 1)
        return fail(FPE_E_INVALID_ARG, "a scan state is canonical: start index (0, 0), row-major");
    FPE_HIP(hipSetDevice(h->device));
    fpe_scan_state* s = new (std::nothrow) fpe_scan_state();
    if (!s) return fail(FPE_E_NOMEM, "out of host memory");
    s->h = h;
    s->g = fpe::make_geom(geom->rows, geom->cols, geom->resolution, geom->position[0], geom->position[1]);
    s->n = static_cast<size_t>(geom->rows) * geom->cols;
    hipError_t e = hipSuccess;
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
        e = hipMalloc(reinterpret_cast<void**>(&s->elev[k]), s->n * sizeof(float) + kLayerPadBytes);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s->var[k]), s->n * sizeof(float) + kLayerPadBytes);
    }
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s->cells), s->n * sizeof(fpe::ScanCell));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s->acc), (fpe::kScanAccWords + 32) * sizeof(int32_t));
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s->own, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->last, hipEventDisableTiming);
    if (e == hipSuccess) e = fpe::launch_scan_set(nullptr, nullptr, reinterpret_cast<uint32_t*>(s->elev[0]), reinterpret_cast<uint32_t*>(s->var[0]), s->n, s->own);
    if (e == hipSuccess) e = fpe::launch_scan_reset(s->cells, s->n, s->acc, s->own);
    if (e == hipSuccess) e = hipEventRecord(s->last, s->own);
    if (e == hipSuccess) e = hipStreamSynchronize(s->own);
    if (e != hipSuccess) {
        fpe_scan_destroy(s);
        return fail_hip(e, "fpe_scan_create");
    }
    *out = s;
    return FPE_OK;
}

int fpe_scan_destroy(fpe_scan_handle s) {
    if (!s) return FPE_OK;
    (void)hipSetDevice(s->h->device);
    if (s->last) (void)hipEventSynchronize(s->last);  // the last operation, on whatever stream it ran
    if (s->own) (void)hipStreamSynchronize(s->own);
    for (int k = 0; k < 2; ++k) {
        if (s->elev[k]) (void)hipFree(s->elev[k]);  // (hipFree synchronises the device: a snapshot update still reading a layer has finished)
        if (s->var[k]) (void)hipFree(s->var[k]);
    }
    if (s->cells) (void)hipFree(s->cells);
    if (s->acc) (void)hipFree(s->acc);
    if (s->rec) (void)hipFree(s->rec);
    if (s->pts) (void)hipFree(s->pts);
    if (s->trav) (void)hipFree(s->trav);
    if (s->closed) (void)hipFree(s->closed);
    if (s->closeAcc) (void)hipFree(s->closeAcc);
    if (s->last) (void)hipEventDestroy(s->last);
    if (s->own) (void)hipStreamDestroy(s->own);
    delete s;
    return FPE_OK;
}

int fpe_scan_geometry(fpe_scan_handle s, fpe_map_desc* out) {
    if (!s || !out) return fail(FPE_E_INVALID_ARG, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    *out = scan_desc(s);
    return FPE_OK;
}

int fpe_scan_set_layers(fpe_scan_handle s, const float* elevation, const float* variance) { return scan_set_layers(s, elevation, variance, false, nullptr); }

int fpe_scan_set_layers_device(fpe_scan_handle s, const float* d_elevation, const float* d_variance, void* stream) {
    return scan_set_layers(s, d_elevation, d_variance, true, static_cast<hipStream_t>(stream));
}

int fpe_scan_read_layers(fpe_scan_handle s, float* elevation, float* variance) { return scan_read_layers(s, elevation, variance, false, nullptr); }

int fpe_scan_read_layers_device(fpe_scan_handle s, float* d_elevation, float* d_variance, void* stream) {
    return scan_read_layers(s, d_elevation, d_variance, true, static_cast<hipStream_t>(stream));
}

int fpe_scan_move(fpe_scan_handle s, const int32_t shift[2], const double position[2], void* stream) {
    if (!s || !shift || !position) return fail(FPE_E_INVALID_ARG, "null argument");
    if (!std::isfinite(position[0]) || !std::isfinite(position[1])) return fail(FPE_E_INVALID_ARG, "bad position");
    std::lock_guard<std::mutex> lk(s->mu);
    ScanOp op{s, static_cast<hipStream_t>(stream)};
    const int rc = op.enter();
    if (rc != FPE_OK) return rc;
    return scan_move_locked(s, shift, position, op.stream);
}

int fpe_scan_fuse(fpe_scan_handle s, const fpe_scan_params* sp, const fpe_scan* scan, const float* points, fpe_scan_info* info) {
    return scan_fuse_common(s, sp, scan, ScanSource::of_points(points), info, false, nullptr);
}

int fpe_scan_fuse_device(fpe_scan_handle s, const fpe_scan_params* sp, const fpe_scan* scan, const float* d_points, fpe_scan_info* d_info, void* stream) {
    return scan_fuse_common(s, sp, scan, ScanSource::of_points(d_points), d_info, true, static_cast<hipStream_t>(stream));
}

int fpe_scan_install(fpe_handle h, fpe_scan_handle s, const fpe_filter_params* fp, void* stream) {
    if (!h || !s) return fail(FPE_E_INVALID_ARG, "null argument");
    if (s->h != h) return fail(FPE_E_INVALID_ARG, "the scan state belongs to another engine");
    fpe_filter_params def;
    if (!fp) {
        fpe::filter_params_defaults(def);
        fp = &def;
    }
    std::lock_guard<std::mutex> lk(s->mu);
    FPE_HIP(hipSetDevice(h->device));
    if (!s->trav) FPE_HIP(hipMalloc(reinterpret_cast<void**>(&s->trav), s->n * sizeof(float) + kLayerPadBytes));
    ScanOp op{s, static_cast<hipStream_t>(stream)};
    int rc = op.enter();
    if (rc != FPE_OK) return rc;
    const fpe_map_desc d = scan_desc(s);
    rc = filters_common(h, &d, fp, s->elev[s->cur], true, s->trav, nullptr, op.stream);
    if (rc != FPE_OK) return rc;
    return upload_common(h, &d, s->trav, s->elev[s->cur], true, op.stream);
}

int fpe_scan_ingest(fpe_handle h, fpe_scan_handle s, const fpe_filter_params* fp, const fpe_scan_params* sp, const fpe_scan* scan, const float* points,
                    const int32_t shift[2], const double position[2], fpe_scan_info* scan_info, fpe_elevation_update_info* update_info) {
    return scan_ingest_common(h, s, fp, sp, nullptr, false, nullptr, false, scan, ScanSource::of_points(points), shift, position, nullptr, scan_info, nullptr, update_info, false, nullptr);
}

int fpe_scan_ingest_device(fpe_handle h, fpe_scan_handle s, const fpe_filter_params* fp, const fpe_scan_params* sp, const fpe_scan* scan,
                           const float* d_points, const int32_t shift[2], const double position[2], fpe_scan_info* d_scan_info,
                           fpe_elevation_update_info* update_info, void* stream) {
    return scan_ingest_common(h, s, fp, sp, nullptr, false, nullptr, false, scan, ScanSource::of_points(d_points), shift, position, nullptr, d_scan_info, nullptr, update_info, true,
                              static_cast<hipStream_t>(stream));
}

int fpe_scan_clear(fpe_scan_handle s, const fpe_scan_params* sp, const fpe_scan_clear_params* cp, const fpe_scan* scan, const float* points,
                   fpe_scan_clear_info* info) {
    return scan_clear_common(s, sp, cp, scan, ScanSource::of_points(points), info, false, nullptr);
}

int fpe_scan_clear_device(fpe_scan_handle s, const fpe_scan_params* sp, const fpe_scan_clear_params* cp, const fpe_scan* scan, const float* d_points,
                          fpe_scan_clear_info* d_info, void* stream) {
    return scan_clear_common(s, sp, cp, scan, ScanSource::of_points(d_points), d_info, true, static_cast<hipStream_t>(stream));
}

int fpe_scan_ingest_clear(fpe_handle h, fpe_scan_handle s, const fpe_filter_params* fp, const fpe_scan_params* sp, const fpe_scan_clear_params* cp,
                          const fpe_scan* scan, const float* points, const int32_t shift[2], const double position[2], fpe_scan_clear_info* clear_info,
                          fpe_scan_info* scan_info, fpe_elevation_update_info* update_info) {
    return scan_ingest_common(h, s, fp, sp, cp, true, nullptr, false, scan, ScanSource::of_points(points), shift, position, clear_info, scan_info, nullptr, update_info, false, nullptr);
}

int fpe_scan_ingest_clear_device(fpe_handle h, fpe_scan_handle s, const fpe_filter_params* fp, const fpe_scan_params* sp, const fpe_scan_clear_params* cp,
                                 const fpe_scan* scan, const float* d_points, const int32_t shift[2], const double position[2],
                                 fpe_scan_clear_info* d_clear_info, fpe_scan_info* d_scan_info, fpe_elevation_update_info* update_info, void* stream) {
    return scan_ingest_common(h, s, fp, sp, cp, true, nullptr, false, scan, ScanSource::of_points(d_points), shift, position, d_clear_info, d_scan_info, nullptr, update_info, true,
                              static_cast<hipStream_t>(stream));
}

int fpe_scan_close(fpe_scan_handle s, const fpe_scan_close_params* kp, const int32_t rect[4], float* out, int64_t out_row_stride, uint8_t* cls,
                   fpe_scan_close_info* info) {
    return scan_close_common(s, kp, rect, out, out_row_stride, cls, info, false, nullptr);
}

int fpe_scan_close_device(fpe_scan_handle s, const fpe_scan_close_params* kp, const int32_t rect[4], float* d_out, int64_t out_row_stride, uint8_t* d_cls,
                          fpe_scan_close_info* d_info, void* stream) {
    return scan_close_common(s, kp, rect, d_out, out_row_stride, d_cls, d_info, true, static_cast<hipStream_t>(stream));
}

int fpe_scan_install_closed(fpe_handle h, fpe_scan_handle s, const fpe_filter_params* fp, const fpe_scan_close_params* kp, void* stream) {
    if (!h || !s) return fail(FPE_E_INVALID_ARG, "null argument");
    if (s->h != h) return fail(FPE_E_INVALID_ARG, "the scan state belongs to another engine");
    fpe_filter_params def;
    if (!fp) {
        fpe::filter_params_defaults(def);
        fp = &def;
    }
    std::lock_guard<std::mutex> lk(s->mu);
    const int32_t whole[4] = {0, 0, s->g.rows, s->g.cols};
    int rc = scan_close_check(s, kp, whole);
    if (rc != FPE_OK) return rc;
    FPE_HIP(hipSetDevice(h->device));
    if (!s->trav) FPE_HIP(hipMalloc(reinterpret_cast<void**>(&s->trav), s->n * sizeof(float) + kLayerPadBytes));
    rc = scan_close_alloc(s);
    if (rc != FPE_OK) return rc;
    ScanOp op{s, static_cast<hipStream_t>(stream)};
    rc = op.enter();
    if (rc != FPE_OK) return rc;
    rc = scan_close_locked(s, kp, whole, s->closed, s->g.cols, nullptr, nullptr, op.stream);
    if (rc != FPE_OK) return rc;
    const fpe_map_desc d = scan_desc(s);
    rc = filters_common(h, &d, fp, s->closed, true, s->trav, nullptr, op.stream);
    if (rc != FPE_OK) return rc;
    return upload_common(h, &d, s->trav, s->closed, true, op.stream);
}

int fpe_scan_ingest_closed(fpe_handle h, fpe_scan_handle s, const fpe_filter_params* fp, const fpe_scan_params* sp, const fpe_scan_clear_params* cp,
                           const fpe_scan_close_params* kp, const fpe_scan* scan, const float* points, const int32_t shift[2], const double position[2],
                           fpe_scan_clear_info* clear_info, fpe_scan_info* scan_info, fpe_scan_close_info* close_info,
                           fpe_elevation_update_info* update_info) {
    return scan_ingest_common(h, s, fp, sp, cp, cp != nullptr, kp, true, scan, ScanSource::of_points(points), shift, position, clear_info, scan_info, close_info, update_info, false,
                              nullptr);
}

int fpe_scan_ingest_closed_device(fpe_handle h, fpe_scan_handle s, const fpe_filter_params* fp, const fpe_scan_params* sp, const fpe_scan_clear_params* cp,
                                  const fpe_scan_close_params* kp, const fpe_scan* scan, const float* d_points, const int32_t shift[2],
                                  const double position[2], fpe_scan_clear_info* d_clear_info, fpe_scan_info* d_scan_info,
                                  fpe_scan_close_info* d_close_info, fpe_elevation_update_info* update_info, void* stream) {
    return scan_ingest_common(h, s, fp, sp, cp, cp != nullptr, kp, true, scan, ScanSource::of_points(d_points), shift, position, d_clear_info, d_scan_info, d_close_info,
                              update_info, true, static_cast<hipStream_t>(stream));
}

// ---- the image forms (point 6 of the scan block): the same routines with an image as the point source ---------------------------
int fpe_scan_fuse_image(fpe_scan_handle s, const fpe_scan_params* sp, const fpe_scan* scan, const fpe_scan_image* im, const void* image,
                        fpe_scan_info* info) {
    return scan_fuse_common(s, sp, scan, ScanSource::of_image(im, image), info, false, nullptr);
}

int fpe_scan_fuse_image_device(fpe_scan_handle s, const fpe_scan_params* sp, const fpe_scan* scan, const fpe_scan_image* im, const void* d_image,
                               fpe_scan_info* d_info, void* stream) {
    return scan_fuse_common(s, sp, scan, ScanSource::of_image(im, d_image), d_info, true, static_cast<hipStream_t>(stream));
}

int fpe_scan_clear_image(fpe_scan_handle s, const fpe_scan_params* sp, const fpe_scan_clear_params* cp, const fpe_scan* scan, const fpe_scan_image* im,
                         const void* image, fpe_scan_clear_info* info) {
    return scan_clear_common(s, sp, cp, scan, ScanSource::of_image(im, image), info, false, nullptr);
}

int fpe_scan_clear_image_device(fpe_scan_handle s, const fpe_scan_params* sp, const fpe_scan_clear_params* cp, const fpe_scan* scan,
                                const fpe_scan_image* im, const void* d_image, fpe_scan_clear_info* d_info, void* stream) {
    return scan_clear_common(s, sp, cp, scan, ScanSource::of_image(im, d_image), d_info, true, static_cast<hipStream_t>(stream));
}

int fpe_scan_ingest_image(fpe_handle h, fpe_scan_handle s, const fpe_filter_params* fp, const fpe_scan_params* sp, const fpe_scan_clear_params* cp,
                          const fpe_scan_close_params* kp, const fpe_scan* scan, const fpe_scan_image* im, const void* image, const int32_t shift[2],
                          const double position[2], fpe_scan_clear_info* clear_info, fpe_scan_info* scan_info, fpe_scan_close_info* close_info,
                          fpe_elevation_update_info* update_info) {
    return scan_ingest_common(h, s, fp, sp, cp, cp != nullptr, kp, kp != nullptr, scan, ScanSource::of_image(im, image), shift, position, clear_info, scan_info,
                              close_info, update_info, false, nullptr);
}

int fpe_scan_ingest_image_device(fpe_handle h, fpe_scan_handle s, const fpe_filter_params* fp, const fpe_scan_params* sp, const fpe_scan_clear_params* cp,
                                 const fpe_scan_close_params* kp, const fpe_scan* scan, const fpe_scan_image* im, const void* d_image,
                                 const int32_t shift[2], const double position[2], fpe_scan_clear_info* d_clear_info, fpe_scan_info* d_scan_info,
                                 fpe_scan_close_info* d_close_info, fpe_elevation_update_info* update_info, void* stream) {
    return scan_ingest_common(h, s, fp, sp, cp, cp != nullptr, kp, kp != nullptr, scan, ScanSource::of_image(im, d_image), shift, position, d_clear_info,
                              d_scan_info, d_close_info, update_info, true, static_cast<hipStream_t>(stream));
}

}  // extern "C"
