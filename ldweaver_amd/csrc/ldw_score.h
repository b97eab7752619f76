// The corrected score of a SNP pair (ldweaver_amd.h 22), stated once for the kernels and for the host.
// Plain C++ when no HIP compiler reads it: tests/host/score_check.cpp reads this header with g++ (tests/test_apc_links_host.py).
#pragma once

#ifdef __HIPCC__
#define LDW_SCORE_FN __host__ __device__ __forceinline__
#elif defined(__GNUC__) && !defined(__clang__)
#define LDW_SCORE_FN __attribute__((optimize("fp-contract=off"))) inline   // (g++ has no pragma for it; the attribute holds whatever the command line says)
#else
#define LDW_SCORE_FN inline
#endif

namespace ldw {

// s = mi - w[A] w[B]: two IEEE operations, a product and then a difference, never one fused multiply-add.  The product is commutative, so the score does
// not depend on which SNP is the from-SNP.  A NaN value, or inf - inf, gives NaN.
LDW_SCORE_FN double pair_score(double mi, double wa, double wb) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double p = wa * wb;
    return mi - p;
}

}  // namespace ldw
