// Consumers of the link tables (SURVEY.md §8 f rank 4), on the device-resident tables left by ldw_mi_all_pairs:
//
//   ldw_lr_tukey  : numeric core of analyse_long_range_links (R/lr_analyser.R:72-108): Tukey outlier thresholds
//                   q3 + (1.5, 3) IQR of the long-range MI values (stats::quantile type 7), the "top ~5000" fallback
//                   (:97-102), the outlier links lr[MI > min(thresholds)] and the ARACNE pool rbind(lr, sr)[MI > min(thresholds)]
//                   (:106-111); ldw_aracne_device then marks the indirect links.
//   ldw_ldmap     : numeric core of genomewide_LDMap (R/LDSummaryPlot.R:55-106): positions that occur in any link are
//                   ranked, the symmetric sparse MI matrix over those ranks is block-summed with the kernel of .mat()
//                   (:176-178: block k = ranks [k r, (k+1) r), the remainder beyond floor(n / r) r is dropped), divided by r^2,
//                   log10(. + 1e-5), rescaled to [0, 1] (:157-163).
//
// Both are HBM-bound row streaming over (a, b, MI) tables: 16 B per link and pass.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ldw_work.h"
#include "ldw_dev.h"

using namespace ldw;

namespace ldw {

__global__ __launch_bounds__(256) void k_mi_keys(const double *__restrict__ mi, int64_t n, uint64_t *__restrict__ key) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) key[i] = f64_key(mi[i]);
}

// rows with MI > thr: kept rows of `which == 0` go to red_row (in table order: one workgroup-wide ordered append per
// 256-row segment keeps the order deterministic after a prefix over segment counts), all of them to the pool
__global__ __launch_bounds__(256) void k_count_gt(const double *__restrict__ mi, int64_t n, double thr, int64_t *__restrict__ seg_cnt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool keep = i < n && mi[i] > thr;
    const unsigned long long b = __ballot(keep);
    __shared__ int wcnt[4];
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) seg_cnt[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

__global__ __launch_bounds__(256) void k_select_gt(const int32_t *__restrict__ a, const int32_t *__restrict__ b, const double *__restrict__ mi,
                                                   int64_t n, double thr, const int64_t *__restrict__ seg_off, int64_t pool_base,
                                                   int64_t *__restrict__ red_row, int32_t *__restrict__ pool_a,
                                                   int32_t *__restrict__ pool_b, double *__restrict__ pool_mi) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool keep = i < n && mi[i] > thr;
    const unsigned long long bal = __ballot(keep);
    __shared__ int wcnt[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    if (!keep) return;
    int64_t dst = seg_off[blockIdx.x];
    for (int w = 0; w < wave; ++w) dst += wcnt[w];
    dst += __popcll(bal & ((1ull << lane) - 1ull));
    if (red_row) red_row[dst] = i;
    pool_a[pool_base + dst] = a[i];
    pool_b[pool_base + dst] = b[i];
    pool_mi[pool_base + dst] = mi[i];
}

// ---- LD map ----
__global__ __launch_bounds__(256) void k_mark_used(const int32_t *__restrict__ a, const int32_t *__restrict__ b, int64_t n,
                                                   const int32_t *__restrict__ POS, int from, int to, int windowed, int32_t *__restrict__ used,
                                                   const int32_t *__restrict__ slot) {
    // slot (r05; null: the SNP index itself): index of a SNP's position among the sorted DISTINCT positions — POS in any order, positions held by
    // several SNPs counted once, like the reference's sort(unique(c(pos1, pos2))) (R/LDSummaryPlot.R:57)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int32_t x = a[i], y = b[i];
        // positions of ALL links define pos_vec; the window then keeps from < pos < to (R/LDSummaryPlot.R:57-62)
        if (!windowed || (POS[x] > from && POS[x] < to)) used[slot ? slot[x] : x] = 1;
        if (!windowed || (POS[y] > from && POS[y] < to)) used[slot ? slot[y] : y] = 1;
    }
}

// A cell's sum must not depend on the order its links arrive in: two contexts holding the same tables give the same map, bit for bit.  fp64 atomic
// adds do not do that, integer ones do: a value goes into a 128-bit fixed-point accumulator in units of 2^-90 (two 64-bit atomic adds, the carry of
// the low word added to the high one: every carry is counted once whatever the order).  A double below 64 in magnitude — an MI is below 2 — is
// placed to within 2^-91, far below the 1e-5 the map adds before its logarithm, and the accumulator's 37 integer bits hold the sum of 2^31 of them.
// Everything else (a larger value, an infinity, a NaN) takes the fp64 atomic add of `odd`, as every value did before.
constexpr int LDMAP_FRAC = 90;
__device__ __forceinline__ void ldmap_acc(double v, unsigned long long *__restrict__ lo, unsigned long long *__restrict__ hi, double *__restrict__ odd) {
    if (!(fabs(v) < 64.0)) {   // (false for NaN too)
        atomicAdd(odd, v);
        return;
    }
    int e;
    const double f = frexp(fabs(v), &e);                              // |v| = f 2^e, f in [0.5, 1)
    const unsigned long long m = (unsigned long long)ldexp(f, 53);    // |v| = m 2^(e - 53), exact
    const int sh = e - 53 + LDMAP_FRAC;
    unsigned __int128 q = 0;
    if (sh >= 0) q = (unsigned __int128)m << sh;                      // (sh <= 43: |v| < 2^6)
    else if (sh > -55) q = (unsigned __int128)((m + (1ull << (-sh - 1))) >> -sh);
    if (q == 0) return;
    if (v < 0) q = (unsigned __int128)0 - q;
    const unsigned long long ql = (unsigned long long)q, qh = (unsigned long long)(q >> 64);
    const unsigned long long old = atomicAdd(lo, ql);
    const unsigned long long carry = old + ql < old ? 1ull : 0ull;
    if (qh + carry != 0) atomicAdd(hi, qh + carry);
}
// The accumulated sum as a double (two's complement over both words), plus what went past the accumulator.  The read-out rounds: (double)lo keeps 53 of
// the low word's 64 bits and the two halves are added in fp64, so the result is the exact sum to within about one ulp of itself (and 2^-79 absolute) —
// the same for the same accumulator, which is all the map needs.
__device__ __forceinline__ double ldmap_sum(unsigned long long lo, unsigned long long hi, double odd) {
    const double s = ldexp((double)(long long)hi, 64 - LDMAP_FRAC) + ldexp((double)lo, -LDMAP_FRAC);
    return odd == 0.0 ? s : s + odd;
}

__global__ __launch_bounds__(256) void k_ldmap_add(const int32_t *__restrict__ a, const int32_t *__restrict__ b, const double *__restrict__ mi,
                                                   int64_t n, const int32_t *__restrict__ POS, int from, int to, int windowed,
                                                   const int32_t *__restrict__ used, const int32_t *__restrict__ rank, int r, int B,
                                                   double *__restrict__ red, unsigned long long *__restrict__ acc_lo, unsigned long long *__restrict__ acc_hi,
                                                   const int32_t *__restrict__ slot) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int32_t x = a[i], y = b[i];
        if (windowed && !(POS[x] >= from && POS[x] <= to && POS[y] >= from && POS[y] <= to)) continue;   // :66-67
        const int32_t sx = slot ? slot[x] : x, sy = slot ? slot[y] : y;
        if (!used[sx] || !used[sy]) continue;   // a window edge position: no level in pos_vec
        const int bi = rank[sx] / r, bj = rank[sy] / r;
        if (bi >= B || bj >= B) continue;     // ranks beyond floor(n / r) * r fall outside every column of .mat()
        // i, j and j, i (:78-80): a pair inside one block counts twice.  Only the upper triangle is accumulated (the
        // mirror cell gets the same value afterwards), so the map is exactly symmetric whatever order the atomics land in.
        const double v = mi[i];
        const int lo = bi < bj ? bi : bj, hi = bi < bj ? bj : bi;
        const int64_t cell = (int64_t)lo * B + hi;
        ldmap_acc(lo == hi ? v + v : v, acc_lo + cell, acc_hi + cell, red + cell);
    }
}

__global__ __launch_bounds__(256) void k_ldmap_log(const double *__restrict__ red, const unsigned long long *__restrict__ acc_lo,
                                                   const unsigned long long *__restrict__ acc_hi, int B, double inv_r2, double *__restrict__ out,
                                                   double *__restrict__ mm) {
    __shared__ double smin[256], smax[256];
    double lo = 1e300, hi = -1e300;
    const int64_t n = (int64_t)B * B;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / B, col = i - row * B;
        const int64_t cell = row <= col ? row * B + col : col * B + row;
        const double s = ldmap_sum(acc_lo[cell], acc_hi[cell], red[cell]);
        const double v = log10(s * inv_r2 + 1e-5);
        out[i] = v;
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    smin[threadIdx.x] = lo;
    smax[threadIdx.x] = hi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            smin[threadIdx.x] = fmin(smin[threadIdx.x], smin[threadIdx.x + s]);
            smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        mm[2 * blockIdx.x] = smin[0];
        mm[2 * blockIdx.x + 1] = smax[0];
    }
}

// (v - min) / (max - min), a division like .rescale01 (R/LDSummaryPlot.R:157-163): the largest cell is exactly 1 and the smallest exactly 0.  A product
// with 1 / rn is not: (mx - mn) * (1 / (mx - mn)) rounds to 1 - 2^-53 for some rn, and which rn a map meets depends on the order the atomics of
// k_ldmap_add land in.
__global__ __launch_bounds__(256) void k_ldmap_rescale(double *__restrict__ red, int64_t n, double mn, double rn) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) red[i] = (red[i] - mn) / rn;
}

// One stable sort of h_POS gives everything the position-based stages look up: the sorted positions with the SNP of every entry (ldw_links_load:
// the first SNP of a position is the first of its run) and a running rank over the distinct positions (the graph nodes of the LD map and ARACNE, which
// like the reference work on positions: SNPs sharing one are one node).  What the order of POS makes trivial is not built.
int pos_order(ldw_ctx *c) {
    auto &po = c->meta.pos_ord;
    if (c->meta.pos_strict || po.n_slots > 0) return LDW_OK;
    const size_t L = (size_t)c->L;
    std::vector<int32_t> ord(L), srt(L), slot(L);
    for (size_t i = 0; i < L; ++i) ord[i] = (int32_t)i;
    std::stable_sort(ord.begin(), ord.end(), [&](int32_t u, int32_t v) { return c->meta.h_POS[(size_t)u] < c->meta.h_POS[(size_t)v]; });
    int32_t k = -1;
    for (size_t i = 0; i < L; ++i) {
        srt[i] = c->meta.h_POS[(size_t)ord[i]];
        if (i == 0 || srt[i] != srt[i - 1]) ++k;
        slot[(size_t)ord[i]] = k;
    }
    if (int rc = po.slot.reserve(L * 4)) return rc;
    LDW_HIP(hipMemcpyAsync(po.slot.p, slot.data(), L * 4, hipMemcpyHostToDevice, c->stream));
    if (!c->meta.pos_sorted) {
        if (int rc = po.srt.reserve(L * 4)) return rc;
        if (int rc = po.order.reserve(L * 4)) return rc;
        LDW_HIP(hipMemcpyAsync(po.srt.p, srt.data(), L * 4, hipMemcpyHostToDevice, c->stream));
        LDW_HIP(hipMemcpyAsync(po.order.p, ord.data(), L * 4, hipMemcpyHostToDevice, c->stream));
    }
    LDW_HIP(hipStreamSynchronize(c->stream));   // (the vectors go out of scope)
    po.n_slots = (int64_t)k + 1;
    return LDW_OK;
}

int pos_slots(ldw_ctx *c, const int32_t **slot, int64_t *n_nodes) {
    if (int rc = pos_order(c)) return rc;
    *slot = c->meta.pos_strict ? nullptr : c->meta.pos_ord.slot.as<int32_t>();
    *n_nodes = c->meta.pos_strict ? c->L : c->meta.pos_ord.n_slots;
    return LDW_OK;
}

__global__ __launch_bounds__(256) void k_iota32(int32_t *__restrict__ a, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) a[i] = (int32_t)i;
}

int sort_positions(ldw_ctx *c, const int32_t *POS, int64_t L, unsigned end_bit, uint32_t *d_pos, int32_t *iota, uint32_t *spos, int32_t *sidx, void *tmp,
                   size_t tmp_bytes) {
    LDW_HIP(hipMemcpyAsync(d_pos, POS, (size_t)L * 4, hipMemcpyHostToDevice, c->stream));
    LDW_LAUNCH(k_iota32, grid_of(L), dim3(256), 0, c->stream, iota, L);
    LDW_HIP((prim_sort_pairs<uint32_t, int32_t>(tmp, tmp_bytes, d_pos, spos, iota, sidx, (size_t)L, 0, end_bit, c->stream)));
    return LDW_OK;
}

static int links_ready(ldw_ctx *c, const char *who) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(c->meta.have_meta, LDW_ERR_STATE, "%s: ldw_set_snp_meta has not been called", who);
    LDW_REQUIRE(c->links.blk_capacity == 0, LDW_ERR_STATE, "%s: a link pass is still open (ldw_links_end)", who);
    return LDW_OK;
}

// stats::quantile type 7 exactly as R evaluates it: index = 1 + (n - 1) p, lo = floor(index), hi = ceiling(index),
// qs = x[lo]; if (index > lo && x[hi] != qs) qs = (1 - h) qs + h x[hi], h = index - lo   (1-based ranks)
struct Q7 {
    double index;
    int64_t lo, hi;
};
static Q7 q7_ranks(int64_t n, double p) {
    Q7 q;
    q.index = ldw::q7_index((double)(n - 1 > 0 ? n - 1 : 0), p);
    q.lo = (int64_t)std::floor(q.index);
    q.hi = (int64_t)std::ceil(q.index);
    return q;
}
static double q7_value(const Q7 &q, double xlo, double xhi) {
    double qs = xlo;
    if (q.index > (double)q.lo && xhi != qs) {
        const double h = q.index - (double)q.lo;
        qs = ldw::q7_interp(h, qs, xhi);
    }
    return qs;
}

}  // namespace ldw

extern "C" {

int ldw_lr_tukey(ldw_ctx *c, int64_t min_links, const int32_t *sr_a, const int32_t *sr_b, const double *sr_mi, int64_t n_sr_rows,
                 double q13_out[2], double thresholds_out[2], int *fallback_out, int64_t *n_red_out, int64_t *n_pool_out) {
    if (int rc = links_ready(c, "ldw_lr_tukey")) return rc;
    LDW_REQUIRE(q13_out && thresholds_out && fallback_out && n_red_out && n_pool_out, LDW_ERR_ARG, "ldw_lr_tukey: null argument");
    LDW_REQUIRE(n_sr_rows >= 0 && (n_sr_rows == 0 || (sr_a && sr_b && sr_mi)), LDW_ERR_ARG, "ldw_lr_tukey: bad short-range table");
    // the short-range part of the ARACNE pool is what sr_links.tsv holds — the REDUCED set perform_MI_computation returned
    // (srp_max > srp_cutoff, R/computePairwiseMI.R:122,140), not the engine's raw short-range table: the caller hands it in
    const int64_t n = c->links.n_lr, ns = n_sr_rows;
    for (int64_t i = 0; i < ns; ++i)   // host arrays: an index outside the alignment (an NA from R's match() is INT_MIN) must not reach the device
        LDW_REQUIRE(sr_a[i] >= 0 && sr_a[i] < c->L && sr_b[i] >= 0 && sr_b[i] < c->L, LDW_ERR_ARG,
                    "ldw_lr_tukey: short-range row %lld has SNP indices (%d, %d) outside 0..%lld (a position that is not in POS?)", (long long)i, sr_a[i], sr_b[i],
                    (long long)c->L - 1);
    c->kept.drop_flags();   // the kept set changes, and ar_flags is working memory below
    if (ns > 0) {
        if (int rc = c->kept.ar_val.reserve((size_t)ns * 4)) return rc;
        if (int rc = c->kept.ar_val2.reserve((size_t)ns * 4)) return rc;
        if (int rc = c->kept.ar_flags.reserve((size_t)ns * 8)) return rc;
        LDW_HIP(hipMemcpyAsync(c->kept.ar_val.p, sr_a, (size_t)ns * 4, hipMemcpyHostToDevice, c->stream));
        LDW_HIP(hipMemcpyAsync(c->kept.ar_val2.p, sr_b, (size_t)ns * 4, hipMemcpyHostToDevice, c->stream));
        LDW_HIP(hipMemcpyAsync(c->kept.ar_flags.p, sr_mi, (size_t)ns * 8, hipMemcpyHostToDevice, c->stream));
        LDW_HIP(hipStreamSynchronize(c->stream));   // pageable sources
    }
    const int32_t *d_sa = c->kept.ar_val.as<int32_t>(), *d_sb = c->kept.ar_val2.as<int32_t>();
    const double *d_smi = c->kept.ar_flags.as<double>();
    LDW_REQUIRE(n > 0, LDW_ERR_STATE, "ldw_lr_tukey: the long-range table is empty");
    LDW_REQUIRE(n < 2147483647LL, LDW_ERR_SIZE, "ldw_lr_tukey: too many long-range links");
    // ---- sorted MI keys -> order statistics ----
    if (int rc = c->kept.ar_key.reserve((size_t)n * 8)) return rc;
    if (int rc = c->kept.ar_key2.reserve((size_t)n * 8)) return rc;
    LDW_LAUNCH(k_mi_keys, grid_of(n), dim3(256), 0, c->stream, c->links.lr_mi.as<double>(), n, c->kept.ar_key.as<uint64_t>());
    size_t tb = 0;
    LDW_HIP(prim_sort_keys_bytes<uint64_t>((size_t)n, 0, 64, c->stream, &tb));
    if (int rc = c->scratch.reserve(tb)) return rc;
    tb = c->scratch.cap;
    LDW_HIP(prim_sort_keys(c->scratch.p, tb, c->kept.ar_key.as<uint64_t>(), c->kept.ar_key2.as<uint64_t>(), (int)n, 0, 64, c->stream));
    auto order_stats = [&](double p, double &q) -> int {
        const Q7 r = q7_ranks(n, p);
        uint64_t k[2];
        LDW_HIP(hipMemcpyAsync(&k[0], c->kept.ar_key2.as<uint64_t>() + (r.lo - 1), 8, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipMemcpyAsync(&k[1], c->kept.ar_key2.as<uint64_t>() + (r.hi - 1), 8, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipStreamSynchronize(c->stream));
        q = q7_value(r, key_f64(k[0]), key_f64(k[1]));
        return LDW_OK;
    };
    double q1 = 0, q3 = 0;
    if (int rc = order_stats(0.25, q1)) return rc;
    if (int rc = order_stats(0.75, q3)) return rc;
    q13_out[0] = q1;
    q13_out[1] = q3;
    const double iqr = q3 - q1;
    double thr[2] = {q3 + 1.5 * iqr, q3 + 3.0 * iqr};
    // ---- rows above min(thresholds): count per 256-row segment, prefix, ordered select ----
    const int64_t nseg_l = (n + 255) / 256, nseg_s = (ns + 255) / 256;
    if (int rc = c->kept.ar_off.reserve((size_t)(nseg_l + nseg_s + 2) * 8 * 2)) return rc;
    int64_t *cnt_l = c->kept.ar_off.as<int64_t>(), *off_l = cnt_l + nseg_l + 1, *cnt_s = off_l + nseg_l + 1, *off_s = cnt_s + nseg_s + 1;
    auto count_pass = [&](double t, int64_t &n_red, int64_t &n_srp) -> int {
        LDW_LAUNCH(k_count_gt, dim3((unsigned)nseg_l), dim3(256), 0, c->stream, c->links.lr_mi.as<double>(), n, t, cnt_l);
        if (ns > 0) LDW_LAUNCH(k_count_gt, dim3((unsigned)nseg_s), dim3(256), 0, c->stream, d_smi, ns, t, cnt_s);
        size_t sb = 0;
        LDW_HIP(prim_scan_bytes<int64_t>((size_t)nseg_l, c->stream, &sb));
        if (int rc = c->scratch.reserve(sb)) return rc;
        sb = c->scratch.cap;
        LDW_HIP(prim_exclusive_sum(c->scratch.p, sb, cnt_l, off_l, (int)nseg_l, c->stream));
        if (ns > 0) LDW_HIP(prim_exclusive_sum(c->scratch.p, sb, cnt_s, off_s, (int)nseg_s, c->stream));
        int64_t last[4] = {0, 0, 0, 0};
        LDW_HIP(hipMemcpyAsync(&last[0], off_l + nseg_l - 1, 8, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipMemcpyAsync(&last[1], cnt_l + nseg_l - 1, 8, hipMemcpyDeviceToHost, c->stream));
        if (ns > 0) {
            LDW_HIP(hipMemcpyAsync(&last[2], off_s + nseg_s - 1, 8, hipMemcpyDeviceToHost, c->stream));
            LDW_HIP(hipMemcpyAsync(&last[3], cnt_s + nseg_s - 1, 8, hipMemcpyDeviceToHost, c->stream));
        }
        LDW_HIP(hipStreamSynchronize(c->stream));
        n_red = last[0] + last[1];
        n_srp = last[2] + last[3];
        return LDW_OK;
    };
    int64_t n_red = 0, n_srp = 0;
    if (int rc = count_pass(std::min(thr[0], thr[1]), n_red, n_srp)) return rc;
    int fallback = 0;
    if (n_red < min_links && n >= min_links) {   // R/lr_analyser.R:97-102: keep ~5000 top links instead
        fallback = 1;
        double t4 = 0, t5 = 0;
        // with the reference's min_links = 5000 both probabilities are in [0, 1]; clamped for smaller caller-chosen values
        if (int rc = order_stats(std::max(0.0, 1.0 - (1.0 / (double)n) * 4000.0), t4)) return rc;
        if (int rc = order_stats(std::max(0.0, 1.0 - (1.0 / (double)n) * 5000.0), t5)) return rc;
        thr[0] = t4;
        thr[1] = t5;
        if (int rc = count_pass(std::min(thr[0], thr[1]), n_red, n_srp)) return rc;
    }
    const double tmin = std::min(thr[0], thr[1]);
    const int64_t n_pool = n_red + n_srp;
    if (int rc = c->kept.row.reserve((size_t)std::max<int64_t>(n_red, 1) * 8)) return rc;
    if (int rc = c->kept.reserve_pool((size_t)std::max<int64_t>(n_pool, 1))) return rc;
    LDW_LAUNCH(k_select_gt, dim3((unsigned)nseg_l), dim3(256), 0, c->stream, c->links.lr_a.as<int32_t>(), c->links.lr_b.as<int32_t>(),
                       c->links.lr_mi.as<double>(), n, tmin, off_l, (int64_t)0, c->kept.row.as<int64_t>(), c->kept.pool_a.as<int32_t>(),
                       c->kept.pool_b.as<int32_t>(), c->kept.pool_mi.as<double>());
    if (ns > 0)
        LDW_LAUNCH(k_select_gt, dim3((unsigned)nseg_s), dim3(256), 0, c->stream, d_sa, d_sb,
                           d_smi, ns, tmin, off_s, n_red, (int64_t *)nullptr, c->kept.pool_a.as<int32_t>(),
                           c->kept.pool_b.as<int32_t>(), c->kept.pool_mi.as<double>());
    LDW_HIP(hipStreamSynchronize(c->stream));
    c->kept.adopt(n_red, n_pool, true);
    thresholds_out[0] = thr[0];
    thresholds_out[1] = thr[1];
    *fallback_out = fallback;
    *n_red_out = n_red;
    *n_pool_out = n_pool;
    return LDW_OK;
}

}  // extern "C"

namespace ldw {
// ldw_ldmap up to the map on the device: *d_htm = the B x B map in the context's working memory, valid until the next call that uses the
// short-range model's buffers.  want = false: the sizes only; capacity >= 0: refused (LDW_ERR_SIZE) when smaller than B x B.
int ldmap_device(ldw_ctx *c, int32_t reducer, int32_t from, int32_t to, int64_t *n_pos_out, int32_t *reducer_out, int32_t *B_out, bool want,
                 int64_t capacity, const double **d_htm) {
    if (int rc = links_ready(c, "ldw_ldmap")) return rc;
    LDW_REQUIRE(n_pos_out && reducer_out && B_out, LDW_ERR_ARG, "ldw_ldmap: null argument");
    const int windowed = (from != 0 || to != 0) ? 1 : 0;
    LDW_REQUIRE(!windowed || (to > from && from >= 0), LDW_ERR_ARG, "ldw_ldmap: <to> must be greater than <from> and both positive");
    LDW_REQUIRE(reducer >= 0, LDW_ERR_ARG, "ldw_ldmap: reducer must be >= 0 (0 = default)");
    const int64_t nl = c->links.n_lr, ns = c->links.n_sr;
    LDW_REQUIRE(nl + ns > 0, LDW_ERR_STATE, "ldw_ldmap: no links");
    // r05: the rank of a position in pos_vec is its rank among the sorted distinct positions.  With POS strictly ascending (what the reference's parser
    // emits) that is the SNP order; otherwise (any order, repeated positions) through a slot per SNP (ldw::pos_slots).
    const int32_t *d_slot = nullptr;
    int64_t n_nodes = 0;
    if (int rc = pos_slots(c, &d_slot, &n_nodes)) return rc;
    // ---- pos_vec: which SNPs occur in a link, and their rank ----
    if (int rc = c->srm.cnt.reserve((size_t)(n_nodes + 1) * 4 * 2)) return rc;
    int32_t *used = c->srm.cnt.as<int32_t>(), *rank = used + n_nodes + 1;
    LDW_HIP(hipMemsetAsync(used, 0, (size_t)(n_nodes + 1) * 4, c->stream));
    const int32_t *POS = c->meta.POS.as<int32_t>();
    if (nl > 0) LDW_LAUNCH(k_mark_used, grid_of(nl), dim3(256), 0, c->stream, c->links.lr_a.as<int32_t>(), c->links.lr_b.as<int32_t>(), nl, POS, from, to, windowed, used, d_slot);
    if (ns > 0) LDW_LAUNCH(k_mark_used, grid_of(ns), dim3(256), 0, c->stream, c->links.sr_a.as<int32_t>(), c->links.sr_b.as<int32_t>(), ns, POS, from, to, windowed, used, d_slot);
    size_t sb = 0;
    LDW_HIP(prim_scan_bytes<int32_t>((size_t)n_nodes + 1, c->stream, &sb));
    if (int rc = c->scratch.reserve(sb)) return rc;
    sb = c->scratch.cap;
    LDW_HIP(prim_exclusive_sum(c->scratch.p, sb, used, rank, (int)(n_nodes + 1), c->stream));
    int32_t n_pos = 0;
    LDW_HIP(hipMemcpyAsync(&n_pos, rank + n_nodes, 4, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    // reducer = round(length(pos_vec) / 1e3) by default (:83-87); R's round() is half-to-even
    int32_t r = reducer > 0 ? reducer : (int32_t)std::nearbyint((double)n_pos / 1e3);
    *n_pos_out = n_pos;
    *reducer_out = r;
    LDW_REQUIRE(r > 1, LDW_ERR_ARG, "ldw_ldmap: reducer %d <= 1: the reference plots the dense %d x %d matrix unreduced, which this entry "
                "point does not materialise (choose a reducer > 1)", r, n_pos, n_pos);
    const int32_t B = n_pos / r;
    *B_out = B;
    LDW_REQUIRE(B > 0, LDW_ERR_ARG, "ldw_ldmap: reducer %d larger than the %d positions", r, n_pos);
    if (!want) return LDW_OK;   // size query
    LDW_REQUIRE(capacity < 0 || capacity >= (int64_t)B * B, LDW_ERR_SIZE, "ldw_ldmap: capacity %lld < %lld", (long long)capacity, (long long)B * B);
    const int64_t nb = (int64_t)B * B;
    const int rgrid = (int)std::min<int64_t>((nb + 255) / 256, 1024);
    if (int rc = c->srm.q.reserve((size_t)nb * 32 + (size_t)rgrid * 16)) return rc;
    // red: what went past the fixed-point accumulators (k_ldmap_add); acc_lo / acc_hi: their two words
    double *red = c->srm.q.as<double>(), *htm = red + 3 * nb, *mm = htm + nb;
    unsigned long long *acc_lo = reinterpret_cast<unsigned long long *>(red + nb), *acc_hi = acc_lo + nb;
    LDW_HIP(hipMemsetAsync(red, 0, (size_t)nb * 24, c->stream));
    if (nl > 0) LDW_LAUNCH(k_ldmap_add, grid_of(nl), dim3(256), 0, c->stream, c->links.lr_a.as<int32_t>(), c->links.lr_b.as<int32_t>(), c->links.lr_mi.as<double>(), nl, POS, from, to, windowed, used, rank, r, B, red, acc_lo, acc_hi, d_slot);
    if (ns > 0) LDW_LAUNCH(k_ldmap_add, grid_of(ns), dim3(256), 0, c->stream, c->links.sr_a.as<int32_t>(), c->links.sr_b.as<int32_t>(), c->links.sr_mi.as<double>(), ns, POS, from, to, windowed, used, rank, r, B, red, acc_lo, acc_hi, d_slot);
    LDW_LAUNCH(k_ldmap_log, dim3(rgrid), dim3(256), 0, c->stream, red, acc_lo, acc_hi, (int)B, 1.0 / ((double)r * (double)r), htm, mm);
    std::vector<double> hmm((size_t)rgrid * 2);
    LDW_HIP(hipMemcpyAsync(hmm.data(), mm, hmm.size() * 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    double mn = hmm[0], mx = hmm[1];
    for (int i = 1; i < rgrid; ++i) {
        mn = std::min(mn, hmm[2 * i]);
        mx = std::max(mx, hmm[2 * i + 1]);
    }
    const double rn = mx - mn;   // 0 -> NaN everywhere, like .rescale01
    LDW_LAUNCH(k_ldmap_rescale, dim3(rgrid), dim3(256), 0, c->stream, htm, nb, mn, rn);
    *d_htm = htm;
    return LDW_OK;
}
}  // namespace ldw

extern "C" {

int ldw_ldmap(ldw_ctx *c, int32_t reducer, int32_t from, int32_t to, int64_t *n_pos_out, int32_t *reducer_out, int32_t *B_out,
              double *htm_out, int64_t capacity) {
    const double *htm = nullptr;
    if (int rc = ldmap_device(c, reducer, from, to, n_pos_out, reducer_out, B_out, htm_out != nullptr, capacity < 0 ? 0 : capacity, &htm)) return rc;
    if (!htm_out) return LDW_OK;
    LDW_HIP(hipMemcpyAsync(htm_out, htm, (size_t)*B_out * *B_out * 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    return LDW_OK;
}

}  // extern "C"

namespace ldw {
void warm_post() {   // ldw_ctx_reserve: load this translation unit's code object ahead of its first launch
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_mi_keys));
    (void)hipGetLastError();
}
}  // namespace ldw
