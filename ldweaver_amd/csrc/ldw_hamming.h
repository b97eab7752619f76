// What the Hamming stage (ldw_hamming.hip) shares with the other reader of its N x N shared-state counts, the neighbour-joining tree
// (ldw_nj.hip): the working memory of one call, the part of the stage that leaves G and scnt on the device, and how an entry is read.
#pragma once
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "ldw_internal.h"

namespace ldw {

struct HamBufs {   // the working memory of one call (the caller releases it once the stream is idle)
    DevBuf info, Hb, T, dig, um, Gh, rl, scnt, dhdw, tmp;
};

// LDW_HOST_TIMING: the host's wall clock since the call began, one line per lap
struct HamClock {
    const HostClock::Point wall0 = HostClock::now();
    double t_last = 0;
    double ms() const { return HostClock::ms(wall0, HostClock::now()); }
    void lap(const char *what) {
        if (!ldw::host_timing()) return;
        const double t = ms();
        fprintf(stderr, "[ldw host] hamming: %-28s %7.3f ms (+%.3f)\n", what, t, t - t_last);
        t_last = t;
    }
};

struct HamShape {   // of the GEMM hamming_gram queued
    int64_t KR = 0, KWr = 0, Kpad = 0;
};

// The stage up to and including its GEMM, queued on the context's stream: bufs.Gh = the lower-triangular int64 [Npad][Npad] of ldw_hamming.hip's
// header comment (tiles on or below the diagonal; with tile0 >= 0 the strip of 128-sequence row tiles [tile0, tile1) alone), bufs.scnt = c of every
// sequence.  Records ev[0] at its start, ev[4] .. ev[2] around the kernels in front of the GEMM and ev[1] behind it.  The alignment is resident.
int hamming_gram(ldw_ctx *c, HamBufs &bufs, int tile0, int tile1, HamClock &clk, HamShape *shape);

// shared(i, j) from the lower-triangular G (element (t, f) with t <= f is always inside a computed tile)
__device__ __forceinline__ int64_t shared_ij(const int64_t *__restrict__ G, int ld, const int32_t *__restrict__ cnt, int64_t L, int64_t i, int64_t j) {
    const int64_t t = i < j ? i : j, f = i < j ? j : i;
    return L - cnt[i] - cnt[j] + G[t * ld + f];
}

}  // namespace ldw
