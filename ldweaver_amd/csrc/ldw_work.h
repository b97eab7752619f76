// Host-side plumbing shared by the post-processing stages (CDS variation, annotation, link reader, consumers, plots, short-range model): the grid of
// a grid-stride pass, a checked launch, the carving of one working buffer into typed arrays, and the ascending order of the SNP positions.
#pragma once
#include <algorithm>

#include "ldw_carve.h"   // Carve: the carving of one working buffer into typed arrays
#include "ldw_internal.h"
#include "ldw_prim.h"

namespace ldw {

// blocks of 256 threads for a grid-stride pass over n items: 1..16384
inline dim3 grid_of(int64_t n) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 16384))); }

// start a kernel; a refused launch leaves the enclosing function with LDW_ERR_HIP (a kernel name with commas goes in parentheses)
#define LDW_LAUNCH(kernel, grid, block, lds, stream, ...)                  \
    do {                                                                    \
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);  \
        LDW_HIP(hipGetLastError());                                         \
    } while (0)

// ldw_post.hip.  The ascending order of the context's positions, built on first use after they change (one stable sort of h_POS: SNPs of one
// position stay in index order) and kept on the device in ctx->meta.pos_ord: slot / n_slots unless POS ascends strictly, srt / order unless it ascends.
int pos_order(ldw_ctx *ctx);
// The caller's POS (host, L entries, any order) ascending on the device, into arrays the caller carved: spos[k] = the k-th smallest position over
// key bits [0, end_bit), sidx[k] = its SNP (equal positions in index order).  d_pos takes POS as given, iota is working memory, tmp holds
// prim_sort_pairs_bytes<uint32_t, int32_t>(L) bytes.  Asynchronous on the context's stream.
int sort_positions(ldw_ctx *ctx, const int32_t *POS, int64_t L, unsigned end_bit, uint32_t *d_pos, int32_t *iota, uint32_t *spos, int32_t *sidx, void *tmp,
                   size_t tmp_bytes);

}  // namespace ldw
