// The fixed-point rule of the per-SNP MI summary (ldweaver_amd.h 21), stated once for the kernel and for the host.
// Plain C++ when no HIP compiler reads it: tests/host/snpsum_q_check.cpp reads this header with g++ (tests/test_background_host.py).
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define LDW_SNPSUM_FN __host__ __device__ __forceinline__
#else
#define LDW_SNPSUM_FN inline
#endif

namespace ldw {

constexpr int SNPSUM_FRAC = 40;   // fraction bits of a summed value
// q(mi) = llrint(mi * 2^40): the product is an exact scaling by a power of two (a subnormal included), the rounding is to nearest, ties to even
// (v_rndne_f64 on the device, the default rounding mode on the host).  A value that is not finite or has |mi| >= 2^22 adds 0 and sets *refused.
// |q| < 2^62; with MI <= ln 5 (|q| < 2^41) and at most 2^21 partners a SNP's sum stays below 2^62.
LDW_SNPSUM_FN int64_t snpsum_q(double mi, bool *refused) {
    const bool ok = fabs(mi) < 4194304.0;   // (false for a NaN)
    *refused = !ok;
    return (int64_t)rint((ok ? mi : 0.0) * 1099511627776.0);
}

}  // namespace ldw
