// Move-only owners of the GPU resources of libldweaver_amd.so: a device block, a pinned host block, an event, a stream.  Whoever declares
// one owns it; it is given back by the destructor, so no owner keeps a list of what to free.  The live counts behind ldw_resource_report
// are kept here, in the create and free paths.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <atomic>
#include <type_traits>

#include "../../include/ldweaver_amd.h"

namespace ldw {

void set_error(const char *fmt, ...);

// process-wide (ldw_alloc.cpp): device blocks held by DevBufs, pinned host blocks, events, streams the library created
struct OwnCounts {
    std::atomic<int64_t> dev{0}, pinned{0}, events{0}, streams{0};
};
extern OwnCounts g_own;

// grow-only device buffer; the blocks come from and go back to the pool of ldw_alloc.cpp
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            release();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    int reserve(size_t bytes);  // returns LDW_OK / error; contents NOT preserved on growth
    int reserve_keep(size_t bytes, size_t used, hipStream_t s);  // preserves the first `used` bytes
    void release();
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// one pinned host block, grow-only
struct PinnedBuf {
    void *p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    PinnedBuf &operator=(PinnedBuf &&o) noexcept {
        if (this != &o) {
            release();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~PinnedBuf() { release(); }
    // contents NOT preserved on growth; LDW_ERR_HIP "<who>: hipHostMalloc of <bytes> bytes failed" leaves no buffer
    int reserve(size_t bytes, const char *who) { return grow(bytes, 0, who); }
    int reserve_keep(size_t bytes, size_t used) { return grow(bytes, used, "pinned staging"); }   // preserves the first `used` bytes
    int64_t release() {   // bytes freed; nothing may still be copying to or from the block
        const int64_t n = (int64_t)cap;
        if (p) {
            (void)hipHostFree(p);
            --g_own.pinned;
        }
        p = nullptr;
        cap = 0;
        return n;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
    operator void *() const { return p; }

private:
    int grow(size_t bytes, size_t used, const char *who) {
        if (bytes <= cap && p) return LDW_OK;
        void *np = nullptr;
        if (!used) release();   // (nothing to keep: the old block goes first)
        if (hipHostMalloc(&np, bytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();   // (the error is sticky; np may hold anything)
            set_error("%s: hipHostMalloc of %zu bytes failed", who, bytes);
            return LDW_ERR_HIP;
        }
        ++g_own.pinned;
        if (p) {
            memcpy(np, p, used);
            release();
        }
        p = np;
        cap = bytes;
        return LDW_OK;
    }
};

// two pinned host buffers of one size: the double buffer of a streaming stage (FASTA feeder, alignment writer, text-file pass)
struct PinnedPair {
    PinnedBuf b[2];
    size_t cap = 0;   // bytes of each
    int reserve(size_t bytes, const char *who) {   // as PinnedBuf::reserve; a failure leaves neither
        if (bytes <= cap) return LDW_OK;
        release();
        for (PinnedBuf &q : b)
            if (int rc = q.reserve(bytes, who)) {
                release();
                return rc;
            }
        cap = bytes;
        return LDW_OK;
    }
    int64_t release() {
        cap = 0;
        return b[0].release() + b[1].release();
    }
};

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event &operator=(Event &&o) noexcept {
        if (this != &o) {
            destroy();
            e = o.e;
            o.e = nullptr;
        }
        return *this;
    }
    ~Event() { destroy(); }
    hipError_t ensure(unsigned flags = hipEventDefault) {   // created on first use
        if (e) return hipSuccess;
        const hipError_t rc = hipEventCreateWithFlags(&e, flags);
        if (rc != hipSuccess) e = nullptr;
        else ++g_own.events;
        return rc;
    }
    void destroy() {
        if (e) {
            (void)hipEventDestroy(e);
            --g_own.events;
        }
        e = nullptr;
    }
    operator hipEvent_t() const { return e; }
};

// an array of Events read as the array of their handles (the launchers take `const hipEvent_t *`: some callers pass handles they do not own)
static_assert(sizeof(Event) == sizeof(hipEvent_t) && std::is_standard_layout<Event>::value, "an Event is its handle and nothing else");
inline const hipEvent_t *handles(const Event *first) { return &first->e; }

// a stream the library created, or one the caller handed in (adopt): that one is never destroyed here
struct Stream {
    hipStream_t s = nullptr;
    bool own = true;
    Stream() = default;
    Stream(Stream &&o) noexcept : s(o.s), own(o.own) { o.s = nullptr, o.own = true; }
    Stream &operator=(Stream &&o) noexcept {
        if (this != &o) {
            destroy();
            s = o.s, own = o.own;
            o.s = nullptr, o.own = true;
        }
        return *this;
    }
    ~Stream() { destroy(); }
    hipError_t ensure(unsigned flags) { return s ? hipSuccess : made(hipStreamCreateWithFlags(&s, flags)); }
    hipError_t ensure(unsigned flags, int priority) { return s ? hipSuccess : made(hipStreamCreateWithPriority(&s, flags, priority)); }
    void adopt(hipStream_t theirs) {
        destroy();
        s = theirs;
        own = false;
    }
    void destroy() {   // nothing may be queued on it
        if (s && own) {
            (void)hipStreamDestroy(s);
            --g_own.streams;
        }
        s = nullptr;
        own = true;
    }
    operator hipStream_t() const { return s; }

private:
    hipError_t made(hipError_t rc) {
        if (rc != hipSuccess) s = nullptr;
        else ++g_own.streams;
        return rc;
    }
};

template <class T> constexpr bool move_only = !std::is_copy_constructible<T>::value && !std::is_copy_assignable<T>::value &&
                                              std::is_move_constructible<T>::value && std::is_move_assignable<T>::value;
static_assert(move_only<DevBuf> && move_only<PinnedBuf> && move_only<Event> && move_only<Stream>, "the owning types move, they are never copied");

}  // namespace ldw
