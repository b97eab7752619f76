// CDS variation and the SNP paint of estimate_variation_in_CDS (R/estimateCDSDiversity.R:27-123) and painter (:151-210).
//
//   ldw_cds_variation : per SNP the counts of the non-reference states (the resident ACGTN_table masked by .ACGTN2num's rule, acgtn_row in
//                       ldw_dev.h), their sum snp_var (int64) and the 5-bit ALT mask; the positions sorted with their index, an exclusive
//                       scan of snp_var in that order, and per CDS two binary searches and ONE fp64 division of an exact integer sum by the
//                       width: the reference's sum(snp_var[pos_idx]) / width is a sum of integers below 2^53, so the value is bit-identical.
//   ldw_cds_paint     : the kept CDSs stabbed into the sorted SNPs with STRICT bounds (start < POS < end), one thread per covered
//                       (CDS, SNP) pair over a flat grid, atomicMax of the label (the reference's loop over labels in ascending order lets the
//                       largest label win); scattered to index order, then the run-length pass of painter on the device: run flags, a scan,
//                       the compacted runs (value, begin), the first / last run fixes of region_mat, and one fill per SNP of the interior 0 runs.
//
// Every L-sized pass is O(L + covered pairs); nothing is k x L.  All global writes are vector stores or vector atomics.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ldw_work.h"
#include "ldw_dev.h"

using namespace ldw;

namespace {

// per SNP: ref = ref_seq[POS - 1]; the ACGTN_table column with the reference row zeroed (.ACGTN2num); its sum and the states left > 0.
__global__ __launch_bounds__(256) void k_cds_snp(const int32_t *__restrict__ counts, const uint32_t *__restrict__ pos, const char *__restrict__ ref,
                                                 int64_t L, int64_t *__restrict__ snp_var, uint8_t *__restrict__ alt, char *__restrict__ refc) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < L; i += (int64_t)gridDim.x * 256) {
        const char ch = ref[pos[i] - 1];
        const int row = acgtn_row(ch);
        int64_t v = 0;
        uint32_t m = 0;
#pragma unroll
        for (int x = 0; x < 5; ++x) {
            const int32_t c = x == row ? 0 : counts[i * 5 + x];
            v += c;
            m |= (c > 0 ? 1u : 0u) << x;
        }
        snp_var[i] = v;
        alt[i] = (uint8_t)m;
        refc[i] = ch;
    }
}

// snp_var in position order, and a 0 at [L] so that the exclusive scan over L + 1 entries ends in the total
__global__ __launch_bounds__(256) void k_cds_gather(const int32_t *__restrict__ sidx, const int64_t *__restrict__ snp_var, int64_t L,
                                                    int64_t *__restrict__ vs) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k <= L; k += (int64_t)gridDim.x * 256) vs[k] = k < L ? snp_var[sidx[k]] : 0;
}

// var_estimate[j] = sum(snp_var : start <= POS <= end) / (end - start + 1); NaN when no SNP falls inside (R's NA)
__global__ __launch_bounds__(256) void k_cds_var(const uint32_t *__restrict__ spos, int64_t L, const int64_t *__restrict__ P,
                                                 const int32_t *__restrict__ starts, const int32_t *__restrict__ ends, int64_t ncds,
                                                 double *__restrict__ var) {
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < ncds; j += (int64_t)gridDim.x * 256) {
        const int64_t s = starts[j], e = ends[j];
        const int64_t lo = lower_bound_dev<int64_t>(spos, L, s), hi = upper_bound_dev<int64_t>(spos, L, e);
        var[j] = (e < s || hi <= lo) ? __builtin_nan("") : (double)(P[hi] - P[lo]) / (double)(e - s + 1);
    }
}

// the sorted SNPs strictly inside kept CDS j: [lo, lo + n); n[nkept] = 0 closes the scan
__global__ __launch_bounds__(256) void k_cds_span(const uint32_t *__restrict__ spos, int64_t L, const int32_t *__restrict__ starts,
                                                  const int32_t *__restrict__ ends, int64_t nkept, int64_t *__restrict__ lo_out,
                                                  int64_t *__restrict__ n_out) {
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j <= nkept; j += (int64_t)gridDim.x * 256) {
        if (j == nkept) {
            n_out[j] = 0;
            continue;
        }
        const int64_t lo = upper_bound_dev<int64_t>(spos, L, starts[j]), hi = lower_bound_dev<int64_t>(spos, L, ends[j]);
        lo_out[j] = lo;
        n_out[j] = hi > lo ? hi - lo : 0;
    }
}

// one thread per covered (CDS, SNP) pair: off = exclusive scan of the spans (off[nkept] = total, read here so the host never waits for it)
__global__ __launch_bounds__(256) void k_cds_stab(const int64_t *__restrict__ off, int64_t nkept, const int64_t *__restrict__ lo,
                                                  const int32_t *__restrict__ label, int32_t *__restrict__ ps) {
    const int64_t total = off[nkept];
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t j = upper_bound_dev<int64_t>(off, nkept + 1, t) - 1;   // the CDS whose span holds t (empty spans share an offset and are skipped)
        atomicMax(ps + lo[j] + (t - off[j]), label[j]);
    }
}

// paint back to SNP index order
__global__ __launch_bounds__(256) void k_cds_scatter(const int32_t *__restrict__ sidx, const int32_t *__restrict__ ps, int64_t L,
                                                     int32_t *__restrict__ p) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < L; k += (int64_t)gridDim.x * 256) p[sidx[k]] = ps[k];
}

// run starts in index order; [L] is a start too, so that the scan's last entry counts the runs and the compaction leaves rbeg[runs] = L
__global__ __launch_bounds__(256) void k_run_flags(const int32_t *__restrict__ p, int64_t L, int32_t *__restrict__ f) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i <= L; i += (int64_t)gridDim.x * 256)
        f[i] = (i == 0 || i == L || p[i] != p[i - 1]) ? 1 : 0;
}

// region_mat: value and first SNP of every run; st[1] counts the runs with a non-zero value
__global__ __launch_bounds__(256) void k_run_compact(const int32_t *__restrict__ p, const int32_t *__restrict__ f, const int32_t *__restrict__ ex,
                                                     int64_t L, int32_t *__restrict__ rbeg, int32_t *__restrict__ rval, int32_t *__restrict__ st) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i <= L; i += (int64_t)gridDim.x * 256) {
        if (!f[i]) continue;
        const int32_t v = i < L ? p[i] : 0;
        rbeg[ex[i]] = (int32_t)i;
        rval[ex[i]] = v;
        if (v != 0) atomicAdd(st + 1, 1);
    }
}

// one thread: the runs painter records (reference: not a last run of one SNP that differs from its predecessor, the `break` at
// i == length(paint)), whether one of them is painted, and the two edge fixes of region_mat in the reference's order.  st[0] = recorded runs.
__global__ void k_run_fix(const int32_t *__restrict__ ex, int64_t L, const int32_t *__restrict__ rbeg, int32_t *__restrict__ rval, int quirk_mode,
                          int32_t *__restrict__ st) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int32_t runs = ex[L];
    const bool drop = quirk_mode == LDW_QUIRK_REFERENCE && runs >= 2 && rbeg[runs - 1] == (int32_t)(L - 1);
    const int32_t m = runs - (drop ? 1 : 0);
    const int32_t nz = st[1] - ((drop && rval[runs - 1] != 0) ? 1 : 0);
    st[0] = m;
    st[1] = nz;
    if (nz == 0) return;
    if (rval[0] == 0) rval[0] = rval[1];             // starting SNPs not labelled: the label from the right
    if (rval[m - 1] == 0) rval[m - 1] = rval[m - 2]; // ending SNPs not labelled: the label from the left
}

// R's round() of (e - b) / 2 for an integer d = e - b >= 1: halves go to the even neighbour
__device__ __forceinline__ int32_t half_round_even(int32_t d) {
    const int32_t q = d >> 1;
    return (d & 1) == 0 ? q : ((q & 1) ? q + 1 : q);
}

// every SNP of a recorded run takes the run's (fixed) value; an interior 0 run [b, e] takes the left value when b == e, else the left value on
// [b, b + ss] and the right one on [b + ss + 1, e], ss = round((e - b) / 2).  The neighbours are read from region_mat, so fills do not cascade.
// SNPs of the unrecorded last run keep their paint.  st[2] counts the SNPs left at 0.
__global__ __launch_bounds__(256) void k_run_fill(const int32_t *__restrict__ p, int64_t L, const int32_t *__restrict__ f,
                                                  const int32_t *__restrict__ ex, const int32_t *__restrict__ rbeg, const int32_t *__restrict__ rval,
                                                  int32_t *__restrict__ st, int32_t *__restrict__ out) {
    const int32_t m = st[0], nz = st[1];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < L; i += (int64_t)gridDim.x * 256) {
        const int32_t r = ex[i] + f[i] - 1;
        int32_t v = p[i];
        if (nz > 0 && r < m) {
            v = rval[r];
            if (v == 0) {
                const int32_t b = rbeg[r], e = rbeg[r + 1] - 1;
                v = (b == e || (int32_t)i <= b + half_round_even(e - b)) ? rval[r - 1] : rval[r + 1];
            }
        }
        out[i] = v;
        if (v == 0) atomicAdd(st + 2, 1);
    }
}

}  // namespace

extern "C" {

int ldw_cds_variation(ldw_ctx *c, const int32_t *POS, int64_t L, const char *ref_seq, int64_t g, const int32_t *cds_start, const int32_t *cds_end,
                      int64_t ncds, double *var_out, int64_t *snp_var_out, uint8_t *alt_mask_out, char *ref_out) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(ldw::have_alignment(c), LDW_ERR_STATE, "ldw_cds_variation: no alignment resident");
    LDW_REQUIRE(POS && ref_seq, LDW_ERR_ARG, "ldw_cds_variation: null argument");
    LDW_REQUIRE(L == c->L, LDW_ERR_ARG, "ldw_cds_variation: L = %lld but the resident alignment has %lld SNPs", (long long)L, (long long)c->L);
    LDW_REQUIRE(g >= 1 && g < ((int64_t)1 << 31), LDW_ERR_ARG, "ldw_cds_variation: reference length %lld outside 1..2^31-1", (long long)g);
    LDW_REQUIRE(ncds >= 0 && ncds < ((int64_t)1 << 31), LDW_ERR_ARG, "ldw_cds_variation: ncds %lld out of range", (long long)ncds);
    LDW_REQUIRE(ncds == 0 || (cds_start && cds_end && var_out), LDW_ERR_ARG, "ldw_cds_variation: null argument");
    for (int64_t i = 0; i < L; ++i)
        LDW_REQUIRE(POS[i] >= 1 && POS[i] <= g, LDW_ERR_ARG, "ldw_cds_variation: POS[%lld] = %d outside 1..%lld", (long long)i, POS[i], (long long)g);
    if (int rc = launch_state_counts(c)) return rc;

    unsigned end_bit = 1;
    while (end_bit < 32 && ((uint64_t)1 << end_bit) <= (uint64_t)g) ++end_bit;
    size_t sort_bytes = 0, scan_bytes = 0;
    LDW_HIP((prim_sort_pairs_bytes<uint32_t, int32_t>((size_t)L, 0, end_bit, c->stream, &sort_bytes)));
    LDW_HIP(prim_scan_bytes<int64_t>((size_t)L + 1, c->stream, &scan_bytes));
    Carve cv;
    auto d_pos = cv.take<uint32_t>(L);
    auto d_ref = cv.take<char>(g);
    auto d_se = cv.take<int32_t>(2 * ncds);
    auto d_var = cv.take<double>(ncds);
    auto d_sv = cv.take<int64_t>(L);
    auto d_alt = cv.take<uint8_t>(L);
    auto d_rc = cv.take<char>(L);
    auto d_iota = cv.take<int32_t>(L);
    auto d_vs = cv.take<int64_t>(L + 1), d_P = cv.take<int64_t>(L + 1);
    auto tmp = cv.take<char>((int64_t)std::max(sort_bytes, scan_bytes));
    if (int rc = cv.reserve(c->cds_work)) return rc;
    if (int rc = c->cds_keep.reserve((size_t)L * 8)) return rc;
    uint32_t *spos = c->cds_keep.as<uint32_t>();
    int32_t *sidx = c->cds_keep.as<int32_t>() + L;
    c->cds_L = 0;

    LDW_HIP(hipMemcpyAsync(d_ref, ref_seq, (size_t)g, hipMemcpyHostToDevice, c->stream));
    if (ncds > 0) {
        LDW_HIP(hipMemcpyAsync(d_se, cds_start, (size_t)ncds * 4, hipMemcpyHostToDevice, c->stream));
        LDW_HIP(hipMemcpyAsync(d_se + ncds, cds_end, (size_t)ncds * 4, hipMemcpyHostToDevice, c->stream));
    }
    if (int rc = sort_positions(c, POS, L, end_bit, d_pos, d_iota, spos, sidx, tmp, sort_bytes)) return rc;
    LDW_LAUNCH(k_cds_snp, grid_of(L), dim3(256), 0, c->stream, c->rows.counts.as<int32_t>(), d_pos, d_ref, L, d_sv, d_alt, d_rc);
    LDW_LAUNCH(k_cds_gather, grid_of(L + 1), dim3(256), 0, c->stream, sidx, d_sv, L, d_vs);
    LDW_HIP((prim_exclusive_sum<int64_t>(tmp, scan_bytes, d_vs, d_P, (size_t)L + 1, c->stream)));
    if (ncds > 0) {
        LDW_LAUNCH(k_cds_var, grid_of(ncds), dim3(256), 0, c->stream, spos, L, d_P, d_se, d_se + ncds, ncds, d_var);
        LDW_HIP(hipMemcpyAsync(var_out, d_var, (size_t)ncds * 8, hipMemcpyDeviceToHost, c->stream));
    }
    if (snp_var_out) LDW_HIP(hipMemcpyAsync(snp_var_out, d_sv, (size_t)L * 8, hipMemcpyDeviceToHost, c->stream));
    if (alt_mask_out) LDW_HIP(hipMemcpyAsync(alt_mask_out, d_alt, (size_t)L, hipMemcpyDeviceToHost, c->stream));
    if (ref_out) LDW_HIP(hipMemcpyAsync(ref_out, d_rc, (size_t)L, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    c->cds_L = L;
    return LDW_OK;
}

int ldw_cds_paint(ldw_ctx *c, const int32_t *cds_start, const int32_t *cds_end, const int32_t *label, int64_t nkept, int nclust, int quirk_mode,
                  int32_t *paint_out, int64_t *n_unpainted_out) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(c->cds_L > 0, LDW_ERR_STATE, "ldw_cds_paint: call ldw_cds_variation first");
    LDW_REQUIRE(paint_out, LDW_ERR_ARG, "ldw_cds_paint: null argument");
    LDW_REQUIRE(nkept >= 0 && nkept < ((int64_t)1 << 31), LDW_ERR_ARG, "ldw_cds_paint: nkept %lld out of range", (long long)nkept);
    LDW_REQUIRE(nkept == 0 || (cds_start && cds_end && label), LDW_ERR_ARG, "ldw_cds_paint: null argument");
    LDW_REQUIRE(nclust >= 1 && nclust <= 255, LDW_ERR_ARG, "ldw_cds_paint: nclust %d outside 1..255", nclust);
    LDW_REQUIRE(quirk_mode == LDW_QUIRK_REFERENCE || quirk_mode == LDW_QUIRK_INTENDED, LDW_ERR_ARG, "ldw_cds_paint: unknown quirk_mode %d", quirk_mode);
    for (int64_t j = 0; j < nkept; ++j)
        LDW_REQUIRE(label[j] >= 1 && label[j] <= nclust, LDW_ERR_ARG, "ldw_cds_paint: label[%lld] = %d outside 1..%d", (long long)j, label[j], nclust);
    const int64_t L = c->cds_L;
    const uint32_t *spos = c->cds_keep.as<uint32_t>();
    const int32_t *sidx = c->cds_keep.as<int32_t>() + L;

    size_t scan64 = 0, scan32 = 0;
    LDW_HIP(prim_scan_bytes<int64_t>((size_t)nkept + 1, c->stream, &scan64));
    LDW_HIP(prim_scan_bytes<int32_t>((size_t)L + 1, c->stream, &scan32));
    Carve cv;
    auto d_se = cv.take<int32_t>(3 * nkept);
    auto lo = cv.take<int64_t>(nkept), n = cv.take<int64_t>(nkept + 1), off = cv.take<int64_t>(nkept + 1);
    auto ps = cv.take<int32_t>(L), p = cv.take<int32_t>(L), f = cv.take<int32_t>(L + 1), ex = cv.take<int32_t>(L + 1);
    auto rbeg = cv.take<int32_t>(L + 1), rval = cv.take<int32_t>(L + 1), out = cv.take<int32_t>(L), st = cv.take<int32_t>(4);
    auto tmp = cv.take<char>((int64_t)std::max(scan64, scan32));
    if (int rc = cv.reserve(c->cds_work)) return rc;

    LDW_HIP(hipMemsetAsync(ps, 0, (size_t)L * 4, c->stream));
    LDW_HIP(hipMemsetAsync(st, 0, 16, c->stream));
    if (nkept > 0) {
        LDW_HIP(hipMemcpyAsync(d_se, cds_start, (size_t)nkept * 4, hipMemcpyHostToDevice, c->stream));
        LDW_HIP(hipMemcpyAsync(d_se + nkept, cds_end, (size_t)nkept * 4, hipMemcpyHostToDevice, c->stream));
        LDW_HIP(hipMemcpyAsync(d_se + 2 * nkept, label, (size_t)nkept * 4, hipMemcpyHostToDevice, c->stream));
    }
    LDW_LAUNCH(k_cds_span, grid_of(nkept + 1), dim3(256), 0, c->stream, spos, L, d_se, d_se + nkept, nkept, lo, n);
    LDW_HIP((prim_exclusive_sum<int64_t>(tmp, scan64, n, off, (size_t)nkept + 1, c->stream)));
    LDW_LAUNCH(k_cds_stab, grid_of(L), dim3(256), 0, c->stream, off, nkept, lo, d_se + 2 * nkept, ps);
    LDW_LAUNCH(k_cds_scatter, grid_of(L), dim3(256), 0, c->stream, sidx, ps, L, p);
    LDW_LAUNCH(k_run_flags, grid_of(L + 1), dim3(256), 0, c->stream, p, L, f);
    LDW_HIP((prim_exclusive_sum<int32_t>(tmp, scan32, f, ex, (size_t)L + 1, c->stream)));
    LDW_LAUNCH(k_run_compact, grid_of(L + 1), dim3(256), 0, c->stream, p, f, ex, L, rbeg, rval, st);
    LDW_LAUNCH(k_run_fix, dim3(1), dim3(64), 0, c->stream, ex, L, rbeg, rval, quirk_mode, st);
    LDW_LAUNCH(k_run_fill, grid_of(L), dim3(256), 0, c->stream, p, L, f, ex, rbeg, rval, st, out);
    int32_t h_st[4] = {0, 0, 0, 0};
    LDW_HIP(hipMemcpyAsync(h_st, st, 16, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemcpyAsync(paint_out, out, (size_t)L * 4, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    LDW_REQUIRE(h_st[1] > 0, LDW_ERR_ARG, "ldw_cds_paint: no SNP lies strictly inside a kept CDS (outside the unrecorded last run)");
    if (n_unpainted_out) *n_unpainted_out = h_st[2];
    return LDW_OK;
}

}  // extern "C"
