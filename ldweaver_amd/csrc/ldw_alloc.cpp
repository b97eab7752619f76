// Error plumbing, the process-wide pool of released device blocks and DevBuf: what every translation unit allocates and reports through; no context here.
#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "ldw_internal.h"

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
namespace ldw {
static thread_local char g_err[1024] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int hip_fail(hipError_t e, const char *what, const char *file, int line) {
    set_error("HIP error %d (%s) at %s:%d: %s", (int)e, hipGetErrorString(e), file, line, what);
    return LDW_ERR_HIP;
}

// ---- r05: released device blocks are kept for the next taker (process-wide, per device).  tools/scratch/realloc_probe.cpp: device memory the runtime has to fetch from the driver
// costs up to 40 ms per GB on this stack (4 x 12 GB: 1.9 s, fresh or right after freeing the same amount; under ~16 GB the runtime re-uses what it just freed), so an engine created after
// another one was destroyed — every test, every job of a long session — waited about a second for the 13-19 GB its context reserves.  Blocks of >= 64 MB go to a free list on release and are
// handed out again best-fit (at most a quarter larger than asked for); LDW_DEVPOOL_GB (default 48, 0: off) caps what is kept; a failing hipMalloc flushes the list and tries again;
// ldw_host_trim gives everything back.  A block is given up only after the device has drained (what hipFree does implicitly), so its next owner cannot meet the last one's kernels.
namespace {
struct PoolBlock {
    void *p;
    size_t cap;
    int dev;
};
std::mutex g_pool_mtx;
std::vector<PoolBlock> g_pool;
size_t g_pool_bytes = 0;
constexpr size_t POOL_MIN = (size_t)64 << 20;
size_t pool_limit() {
    static const size_t v = [] {
        const char *e = getenv("LDW_DEVPOOL_GB");
        const double gb = e ? atof(e) : 48.0;
        return gb > 0 ? (size_t)(gb * 1073741824.0) : (size_t)0;
    }();
    return v;
}
void *pool_take(size_t want, size_t &cap_out) {
    if (want < POOL_MIN || pool_limit() == 0) return nullptr;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(g_pool_mtx);
    size_t best = (size_t)-1;
    for (size_t i = 0; i < g_pool.size(); ++i)
        if (g_pool[i].dev == dev && g_pool[i].cap >= want && g_pool[i].cap <= want + want / 4 && (best == (size_t)-1 || g_pool[i].cap < g_pool[best].cap)) best = i;
    if (best == (size_t)-1) return nullptr;
    void *p = g_pool[best].p;
    cap_out = g_pool[best].cap;
    g_pool_bytes -= cap_out;
    g_pool[best] = g_pool.back();
    g_pool.pop_back();
    return p;
}
// r06: a caller that has drained every stream that could touch its blocks (ldw_ctx_destroy: the context's own streams) says so for the
// duration of its releases, and the device-wide synchronisation — which stalls OTHER contexts of the device in the middle of their passes — is skipped
thread_local bool g_owner_drained = false;
std::atomic<int> g_live_ctx{0};
size_t pool_idle_limit() {   // what the free list may keep once the process holds no context at all (LDW_DEVPOOL_IDLE_GB, default 24; the live cap is LDW_DEVPOOL_GB)
    static const size_t v = [] {
        const char *e = getenv("LDW_DEVPOOL_IDLE_GB");
        const double gb = e ? atof(e) : 24.0;
        return gb > 0 ? (size_t)(gb * 1073741824.0) : (size_t)0;
    }();
    return v;
}
// a block goes back to the runtime: large ones zero-filled first (the runtime may hand the same memory to the next hipMalloc without clearing it;
// the pages are mapped, so this runs at HBM speed), so that whatever dev_alloc gets from the runtime reads as zero
void pool_free_zeroed(void *p, size_t cap) {
    if (cap >= POOL_MIN && hipMemsetAsync(p, 0, cap, nullptr) != hipSuccess) (void)hipGetLastError();
    (void)hipFree(p);   // (waits for the fill)
}
void pool_give(void *p, size_t cap) {
    if (!p) return;
    if (cap >= POOL_MIN && pool_limit() > 0) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, p) == hipSuccess) {
            int cur = 0;
            (void)hipGetDevice(&cur);
            if (cur != at.device) (void)hipSetDevice(at.device);
            const bool drained = g_owner_drained || hipDeviceSynchronize() == hipSuccess;   // (the releasing context's kernels are done with it: what hipFree waits for as well)
            if (cur != at.device) (void)hipSetDevice(cur);
            if (drained) {
                std::lock_guard<std::mutex> lk(g_pool_mtx);
                if (g_pool_bytes + cap <= pool_limit()) {
                    g_pool.push_back(PoolBlock{p, cap, at.device});
                    g_pool_bytes += cap;
                    return;
                }
            }
        }
        (void)hipGetLastError();
    }
    pool_free_zeroed(p, cap);
}
// keep: bytes the list may hold afterwards (0: give everything back); the largest blocks go first
size_t pool_flush(size_t keep = 0) {
    std::vector<PoolBlock> all;
    {
        std::lock_guard<std::mutex> lk(g_pool_mtx);
        if (keep == 0) {
            all.swap(g_pool);
            g_pool_bytes = 0;
        } else {
            std::sort(g_pool.begin(), g_pool.end(), [](const PoolBlock &x, const PoolBlock &y) { return x.cap < y.cap; });
            while (g_pool_bytes > keep && !g_pool.empty()) {
                all.push_back(g_pool.back());
                g_pool_bytes -= g_pool.back().cap;
                g_pool.pop_back();
            }
        }
    }
    size_t n = 0;
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (const PoolBlock &b : all) {
        (void)hipSetDevice(b.dev);
        pool_free_zeroed(b.p, b.cap);
        n += b.cap;
    }
    if (!all.empty()) (void)hipSetDevice(cur);
    return n;
}
// a block of at least `want` bytes: from the free list, else from the runtime (a second try after giving the free list back)
// LDW_POISON_ALLOC=1 (debugging aid, any build): every block handed out is filled with 0xA5 first — fresh device memory happens to be zero on this stack, a block from
// the free list (or from the runtime's own cache) is not, and code that reads what it never wrote must not depend on the difference (tools/fuzz_paths.py found one such read)
bool poison_on() {
    static const bool on = getenv("LDW_POISON_ALLOC") != nullptr;
    return on;
}
// LDW_POISON_ALLOC=1: bytes 0xA5 (an index read from it is wild: the kernel faults).  LDW_POISON_ALLOC=2: int32 words of 1 — indices stay in range, flags
// read "set", floats are denormals: a read-before-write shows as a wrong RESULT instead of a fault (the gentler first probe)
void poison_fill(void *p, size_t bytes) {
    static const int mode = getenv("LDW_POISON_ALLOC") ? atoi(getenv("LDW_POISON_ALLOC")) : 0;
    if (mode == 2) (void)hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(p), 1, bytes / 4);
    else if (mode == 3) (void)hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(p), 0x00000A5A, bytes / 4);   // a second in-range pattern: index 2650, flags set, float denormal
    else (void)hipMemset(p, 0xA5, bytes);
    (void)hipDeviceSynchronize();
}
hipError_t dev_alloc(void **out, size_t want, size_t &cap_out) {
    if (void *p = pool_take(want, cap_out)) {
        // a block from the free list holds its last owner's data; memory that comes from the driver is zero, and the engine has always been handed zeroed
        // blocks (nothing else was ever observed on this stack): keep it so — LDW_POISON_ALLOC (below) found kernels that read index arrays before writing
        // them, which zeroes make harmless and another buffer's contents would not.  The pages are mapped already: the fill runs at HBM speed (7 ms for 20 GB).
        hipError_t e = hipMemsetAsync(p, 0, cap_out, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);   // (the library's streams do not synchronise with the null stream; only the fill has to be done — no device-wide wait)
        if (e == hipSuccess && poison_on()) poison_fill(p, cap_out);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(p);
        } else {
            *out = p;
            return hipSuccess;
        }
    }
    hipError_t e = hipMalloc(out, want);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (pool_flush() > 0) e = hipMalloc(out, want);
    }
    cap_out = want;
    // r06 — "a fresh DevBuf reads as zero" as an invariant with a reason per source, instead of an accident of the stack:
    //   * from the free list: zero-filled above (mapped pages: HBM speed);
    //   * small blocks (< 64 MB, never pooled: the runtime caches and re-uses them DIRTY): zero-filled here, microseconds;
    //   * large blocks from the runtime: either fresh from the driver — the kernel driver clears VRAM it hands to a process — or a block this library
    //     gave back with hipFree, and those are zero-filled BEFORE they are freed (pool_free_zeroed).  Filling them here as well was measured: it maps
    //     every page of the 13-19 GB a context reserves (0.37 s on a job's first Hamming call against 6 ms: profiles/r06_alloc_zero_fill.txt).
    // It is NOT what makes stale data harmless: a DevBuf kept across problems holds the last problem's bytes; tools/fuzz_paths.py and tests/test_bounds.py
    // run ~500 problems one after the other on one context for that, LDW_POISON_ALLOC=2 / 3 fill every block with in-range garbage instead of zeroes.
    if (e == hipSuccess && want < POOL_MIN) {
        e = hipMemsetAsync(*out, 0, want, nullptr);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(*out);
            *out = nullptr;
        }
    }
    if (e == hipSuccess && poison_on()) poison_fill(*out, want);
    return e;
}
}  // namespace

OwnCounts g_own;
size_t device_pool_trim() { return pool_flush(); }
void ctx_count(int d) {
    if (g_live_ctx.fetch_add(d) + d <= 0 && d < 0) (void)pool_flush(pool_idle_limit() ? pool_idle_limit() : 0);   // the last context of the process has gone
}
DrainedScope::DrainedScope() { g_owner_drained = true; }
DrainedScope::~DrainedScope() { g_owner_drained = false; }

int DevBuf::reserve(size_t bytes) {
    if (bytes <= cap && p) return LDW_OK;
    release();
    size_t want = bytes < 256 ? 256 : bytes, got = 0;
    LDW_HIP(dev_alloc(&p, want, got));
    ++g_own.dev;
    cap = got;
    return LDW_OK;
}

int DevBuf::reserve_keep(size_t bytes, size_t used, hipStream_t s) {
    if (bytes <= cap && p) return LDW_OK;
    size_t want = bytes < 256 ? 256 : bytes;
    if (want < cap + cap / 2) want = cap + cap / 2;  // geometric growth for the link tables
    void *np = nullptr;
    size_t got = 0;
    {
        hipError_t e = dev_alloc(&np, want, got);
        if (e != hipSuccess) {
            size_t fr = 0, tot = 0;
            (void)hipMemGetInfo(&fr, &tot);
            set_error("hipMalloc of %zu bytes failed (%s); %zu of %zu bytes free on the device", want, hipGetErrorString(e), fr, tot);
            return LDW_ERR_HIP;
        }
    }
    if (p && used) {
        hipError_t e = hipMemcpyAsync(np, p, used, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            pool_give(np, got);
            return hip_fail(e, "DevBuf::reserve_keep: copy of the kept bytes", __FILE__, __LINE__);
        }
    }
    release();
    ++g_own.dev;
    p = np;
    cap = got;
    return LDW_OK;
}

void DevBuf::release() {
    if (p) {
        pool_give(p, cap);
        --g_own.dev;
    }
    p = nullptr;
    cap = 0;
}
}  // namespace ldw

extern "C" {

const char *ldw_last_error(void) { return ldw::g_err; }

int ldw_resource_report(int64_t out[5]) {
    LDW_REQUIRE(out, LDW_ERR_ARG, "ldw_resource_report: null argument");
    out[0] = ldw::g_own.dev;
    {
        std::lock_guard<std::mutex> lk(ldw::g_pool_mtx);
        out[1] = (int64_t)ldw::g_pool.size();
    }
    out[2] = ldw::g_own.pinned;
    out[3] = ldw::g_own.events;
    out[4] = ldw::g_own.streams;
    return LDW_OK;
}

}  // extern "C"
