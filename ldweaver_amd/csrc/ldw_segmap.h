// The fixed-point rule of the segment map (ldweaver_amd.h 24), stated once for the kernels and for the host.
// Plain C++ when no HIP compiler reads it: tests/host/segmap_q_check.cpp reads this header with g++ (tests/test_segmap_host.py).
#pragma once
#include <math.h>
#include <stdint.h>

#include "ldw_snpsum.h"

#ifdef __HIPCC__
#define LDW_SEGMAP_FN __host__ __device__ __forceinline__
#else
#define LDW_SEGMAP_FN inline
#endif

namespace ldw {

constexpr int SEGMAP_LO_BITS = 24;   // bits of q kept in the low word of a cell's sum
// q(v) = llrint(v * 2^40), snpsum_q's product and rounding, with this entry's own refusal range: a value that is not finite or has |v| >= 4 adds 0 and
// sets *refused.  |q| <= 2^42.
LDW_SEGMAP_FN int64_t segmap_q(double v, bool *refused) {
    const bool ok = fabs(v) < 4.0;   // (false for a NaN)
    *refused = !ok;
    bool never;
    return snpsum_q(ok ? v : 0.0, &never);
}
// q = hi * 2^24 + lo with 0 <= lo < 2^24 (hi is the arithmetic shift, so the identity holds for a negative q).  A cell sums the two words apart: with
// |q| <= 2^42 (|hi| <= 2^18) both sums stay below 2^63 for any cell of fewer than 2^39 pairs.
LDW_SEGMAP_FN void segmap_split(int64_t q, int64_t *lo, int64_t *hi) {
    *lo = q & ((int64_t(1) << SEGMAP_LO_BITS) - 1);
    *hi = q >> SEGMAP_LO_BITS;
}

}  // namespace ldw
