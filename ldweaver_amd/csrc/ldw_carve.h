// The carving of one working buffer into typed arrays (the post-processing stages through ldw_work.h, the per-slot buffers of a block's launch
// chain through ldw_slots.h).  Plain C++, no HIP: tests/host/slot_layout_check.cpp reads it with g++.
#pragma once
#include <algorithm>
#include <cassert>
#include <cstddef>
#include <cstdint>

namespace ldw {

// Bump allocation of one working buffer in 256-byte steps: take<T>(n) names an array of max(n, 1) elements and its element type once; after
// reserve() (or bind(), for a buffer that was reserved before) the Slot it returned converts to the array's T * (pointer arithmetic and calls
// take it as one).  cover(a, b, ..) is the byte range of the arrays it is given, padding included: what a memset of "these arrays" clears — the arrays
// must lie one behind the other with nothing else between them (asserted).
struct Carve {
    template <class T> struct Slot {
        const Carve *cv;
        size_t off, len, n;   // first byte; bytes up to the next array; elements named
        operator T *() const { return reinterpret_cast<T *>(cv->base + off); }
    };
    struct Range {
        char *p;
        size_t bytes;
        unsigned int n16() const { return (unsigned int)(bytes / 16); }   // (k_zero4 clears 16-byte pieces; the steps are multiples of 256)
    };
    size_t bytes = 0;
    char *base = nullptr;
    template <class T> Slot<T> take(int64_t n) {
        const size_t o = bytes;
        bytes += ((size_t)std::max<int64_t>(n, 1) * sizeof(T) + 255) & ~(size_t)255;
        return Slot<T>{this, o, bytes - o, (size_t)std::max<int64_t>(n, 1)};
    }
    template <class Buf> int reserve(Buf &b) {
        const int rc = b.reserve(bytes);
        bind(b);
        return rc;
    }
    template <class Buf> void bind(const Buf &b) { base = b.template as<char>(); }
    template <class... S> Range cover(const S &...s) const {
        const size_t lo = std::min({s.off...}), hi = std::max({(s.off + s.len)...});
        assert((s.len + ...) == hi - lo);
        return Range{base + lo, hi - lo};
    }
};

}  // namespace ldw
