// The 5 x 5 joint table of a SNP pair over a set of sequences and its evaluation: shared by the lineage check (ldw_lineage.hip) and the
// permutation test (ldw_perm.hip).  Integers are exact and the evaluation is this one piece of code, so equal tables give equal bits
// in either file.  Both include it under `#pragma clang fp contract(off)`: the value is then a function of the table alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ldw {

struct LinTable {
    int32_t cnt[25];
    int64_t fix[25];
};

// MI of one table (include/ldweaver_amd.h 18) and its poly flags.  The including file compiles without FMA contraction, so the value is a function of the table.
__device__ __forceinline__ double lin_eval(const LinTable &t, double scale, double neff, uint32_t *poly) {
    int32_t ca[5], cb[5];
    int64_t fa[5], fb[5];
#pragma unroll
    for (int X = 0; X < 5; ++X) ca[X] = cb[X] = 0, fa[X] = fb[X] = 0;
#pragma unroll
    for (int X = 0; X < 5; ++X)
#pragma unroll
        for (int Y = 0; Y < 5; ++Y) {
            ca[X] += t.cnt[X * 5 + Y], cb[Y] += t.cnt[X * 5 + Y];
            fa[X] += t.fix[X * 5 + Y], fb[Y] += t.fix[X * 5 + Y];
        }
    int na = 0, nb = 0;
#pragma unroll
    for (int X = 0; X < 5; ++X) na += ca[X] > 0, nb += cb[X] > 0;
    *poly = (uint32_t)(na > 1) | ((uint32_t)(nb > 1) << 1);
    if (na <= 1 && nb <= 1) return 0.0;   // no member, or both SNPs monomorphic: the formula's log 1, not left to rounding
    const double ra = (double)na, rb = (double)nb;
    const double den = neff + 0.5 * ra * rb, rxy = 0.25 * ra * rb;
    double mi = 0.0;
#pragma unroll
    for (int X = 0; X < 5; ++X) {
        if (ca[X] <= 0) continue;
        const double pX = (double)fa[X] * scale;
#pragma unroll
        for (int Y = 0; Y < 5; ++Y) {
            if (cb[Y] <= 0) continue;
            const double pY = (double)fb[Y] * scale;
            const double pxy = (double)t.fix[X * 5 + Y] * scale + 0.5;
            mi += (pxy / den) * log(pxy / (pX * pY + rxy + 0.5 * ra * pX + 0.5 * rb * pY) * den);
        }
    }
    return mi;
}

__device__ __forceinline__ void lin_zero(LinTable &t) {
#pragma unroll
    for (int q = 0; q < 25; ++q) t.cnt[q] = 0, t.fix[q] = 0;
}
__device__ __forceinline__ void lin_add(LinTable &t, const LinTable &x) {
#pragma unroll
    for (int q = 0; q < 25; ++q) t.cnt[q] += x.cnt[q], t.fix[q] += x.fix[q];
}
// every lane gets the wave's sums of the cells both SNPs can fill
__device__ __forceinline__ void lin_reduce(LinTable &t, uint32_t pa, uint32_t pb) {
#pragma unroll
    for (int X = 0; X < 5; ++X) {
        if (!((pa >> X) & 1u)) continue;
#pragma unroll
        for (int Y = 0; Y < 5; ++Y) {
            if (!((pb >> Y) & 1u)) continue;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                t.cnt[X * 5 + Y] += __shfl_xor(t.cnt[X * 5 + Y], off);
                t.fix[X * 5 + Y] += (int64_t)__shfl_xor((long long)t.fix[X * 5 + Y], off);
            }
        }
    }
}

}  // namespace ldw
