// LD decay (ldweaver_amd.h 20): a 2-D histogram, circular distance bin x MI bucket, over EVERY SNP pair of a block list, with the
// largest MI of every distance bin.  The values are the dense block the plain path writes (block_mi_dense -> ctx->MIblk, column-major), the
// distance is circ_len (ldw_dev.h), the MI bin is mi_bucket (ldw_epi.h) >> mi_shift.  Every output is an integer add or a maximum of an
// order-preserving 64-bit key: no result depends on the order of the adds.
//
// k_decay_hist: a workgroup of four waves takes a patch of 64 rows (a_loc, the lanes: a wave reads 512 contiguous bytes of a column) x
// DEC_C columns (b_loc, wave w takes the columns w, w + 4, ...).  From the extreme positions of its rows and columns it bounds the patch's
// circular distances, hence its distance bins lo..hi (the bin is monotone in the distance), and takes one of two routes:
//   (A) (hi - lo + 1) * NB uint32 counters fit DEC_LDS_CNT: counts with LDS atomics (the lanes that share the first active lane's counter
//       are added as one), then one 64-bit global add per non-zero counter;
//   (B) else: each wave combines the lanes that share a (distance bin, MI bin) key in a readfirstlane / ballot loop and the leader adds the
//       population count to the global counter.
// The bound is taken from 64 + DEC_C positions, not from the patch's pairs: it holds every pair in exact arithmetic, and a pair that rounding
// (a fractional g) puts outside it is added straight to the global counters, so both routes count every pair in its own bin whatever the bound.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <vector>

#include "ldw_internal.h"
#include "ldw_dev.h"
#include "ldw_epi.h"

using namespace ldw;

namespace ldw {

#ifndef LDW_ABLATE_DECAY
#define LDW_ABLATE_DECAY 0   // measurement builds (make VARIANT=.. EXTRA_DEFS=-DLDW_ABLATE_DECAY=n): 1 = count nothing, 2 = no division per pair; DESIGN.md 31
#endif
constexpr int DEC_ROWS = 64;         // rows of a patch: the lanes of a wave
constexpr int DEC_C = 256;           // columns of a patch
constexpr int DEC_THREADS = 256;
constexpr int DEC_WAVES = DEC_THREADS / 64;
constexpr int DEC_U = 8;             // columns a wave has in flight
constexpr int DEC_LDS_CNT = 8192;    // uint32 counters of route A's window (32 KB)
constexpr int DEC_MAX_CUTS = 1023;
static_assert(DEC_C == DEC_THREADS, "every thread fetches the position of one column of the patch");
constexpr int DEC_WIN_MAX = DEC_LDS_CNT / (NBINS >> 6);   // most distance bins of a window (mi_shift 6: 64 MI bins each)

struct DecayArgs {
    const double *MI;               // [nf * nt] column-major: the pair (a_loc, b_loc) at a_loc + b_loc * nf
    int64_t nf, nt;
    const int32_t *pos_f, *pos_t;   // positions of the two sides, read through idx_f / idx_t (null: the local index itself)
    const int32_t *idx_f, *idx_t;
    double g;
    int diag;                       // 1: pairs a_loc > b_loc; 0: pairs a_loc != b_loc
    const double *cuts;
    int n_cut, mi_shift, route;     // route 0: the patch chooses; 1: A or refuse; 2: B
    unsigned long long *hist;       // [(n_cut + 1)][NB]
    unsigned long long *maxkey;     // [n_cut + 1]: f64_key of the largest value, 0 = no pair yet
    unsigned long long *stat;       // [0] patches, [1] patches on route B, [2] pairs outside their patch's bound, [3] patches route 1 refused
};

// number of cuts strictly below len, searched in cuts[l .. h)
__device__ __forceinline__ int cuts_below(const double *cuts, int l, int h, double len) {
    while (l < h) {
        const int mid = (l + h) >> 1;
        if (cuts[mid] < len) l = mid + 1;
        else h = mid;
    }
    return l;
}

__device__ __forceinline__ void max_to_global(unsigned long long *p, unsigned long long key) {
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key) atomicMax(p, key);
}

__global__ __launch_bounds__(DEC_THREADS) void k_decay_hist(DecayArgs A) {
    __shared__ double s_cuts[DEC_MAX_CUTS + 1];
    __shared__ uint32_t s_cnt[DEC_LDS_CNT];
    __shared__ unsigned long long s_max[DEC_WIN_MAX];
    __shared__ int s_ext[4];   // min / max position of the rows, of the columns
    __shared__ int s_pt[DEC_C];   // the positions of the patch's columns
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int NB = NBINS >> A.mi_shift;
    const int64_t a0 = (int64_t)blockIdx.x * DEC_ROWS, b0 = (int64_t)blockIdx.y * DEC_C;
    const int64_t a1 = a0 + DEC_ROWS < A.nf ? a0 + DEC_ROWS : A.nf, b1 = b0 + DEC_C < A.nt ? b0 + DEC_C : A.nt;
    if (A.diag && a1 - 1 <= b0) return;   // no pair a_loc > b_loc in the patch
    for (int i = tid; i < A.n_cut; i += DEC_THREADS) s_cuts[i] = A.cuts[i];
    if (tid == 0) s_ext[0] = s_ext[2] = 0x7FFFFFFF, s_ext[1] = s_ext[3] = (int)0x80000000;
    __syncthreads();
    const int64_t a = a0 + lane;
    const bool row_ok = a < a1;
    const int pf_i = row_ok ? A.pos_f[A.idx_f ? A.idx_f[a] : a] : 0;
    {   // the extremes: rows by wave 0, columns by all (DEC_C == DEC_THREADS)
        int mn = 0x7FFFFFFF, mx = (int)0x80000000;
        if (w == 0 && row_ok) mn = mx = pf_i;
        int tn = 0x7FFFFFFF, tx = (int)0x80000000;
        if (b0 + tid < b1) s_pt[tid] = tn = tx = A.pos_t[A.idx_t ? A.idx_t[b0 + tid] : b0 + tid];
        for (int o = 32; o; o >>= 1) {
            mn = min(mn, __shfl_xor(mn, o)), mx = max(mx, __shfl_xor(mx, o));
            tn = min(tn, __shfl_xor(tn, o)), tx = max(tx, __shfl_xor(tx, o));
        }
        if (lane == 0) {
            if (w == 0) atomicMin(&s_ext[0], mn), atomicMax(&s_ext[1], mx);
            atomicMin(&s_ext[2], tn), atomicMax(&s_ext[3], tx);
        }
    }
    __syncthreads();
    // x = pos1 - pos2 (to side - from side) of the patch lies in [x0, x1]; len(x) is the triangle wave of period g: 0 at the multiples of g, g / 2 half-way
    const double g = A.g, x0 = (double)s_ext[2] - (double)s_ext[1], x1 = (double)s_ext[3] - (double)s_ext[0];
    double lmin = 0.0, lmax = 0.5 * g;
    if (x1 - x0 < g) {
        const double l0 = circ_len(x0, 0.0, g), l1 = circ_len(x1, 0.0, g);
        if (floor(x1 / g) == floor(x0 / g)) lmin = fmin(l0, l1);   // (x0 itself a multiple of g: l0 = 0)
        if (floor((x1 - 0.5 * g) / g) == floor((x0 - 0.5 * g) / g)) lmax = fmax(l0, l1);
    }
    const int lo = cuts_below(s_cuts, 0, A.n_cut, lmin), hi = cuts_below(s_cuts, lo, A.n_cut, lmax);
    const int W = hi - lo + 1;
    const bool fits = W * NB <= DEC_LDS_CNT;
    if (A.route == 1 && !fits) {
        if (tid == 0) atomicAdd(&A.stat[3], 1ull);
        return;
    }
    const bool lds = fits && A.route != 2;
    if (tid == 0) {
        atomicAdd(&A.stat[0], 1ull);
        if (!lds) atomicAdd(&A.stat[1], 1ull);
    }
    if (lds) {
        for (int i = tid; i < W * NB; i += DEC_THREADS) s_cnt[i] = 0;
        if (tid < W) s_max[tid] = 0;
        __syncthreads();
    }
    // a pair whose bin is not in lo..hi shows at the ends of the restricted search: below needs cuts[lo - 1] >= len, above cuts[hi] < len
    const double cut_under = lo > 0 ? s_cuts[lo - 1] : -1.0, cut_top = hi < A.n_cut ? s_cuts[hi] : INFINITY;
    const double pf = (double)pf_i;
    int cur_bin = -1;
    unsigned long long cur_key = 0;
    auto flush_max = [&]() {
        if (cur_bin < 0) return;
        if (lds) {
            if (s_max[cur_bin - lo] < cur_key) atomicMax(&s_max[cur_bin - lo], cur_key);
        } else
            max_to_global(&A.maxkey[cur_bin], cur_key);
    };
    auto count = [&](int64_t b, double mi) {   // the pair (a, b), if it is one, into its counter
        const bool active = row_ok && (A.diag ? a > b : a != b);
        const double pt = (double)s_pt[b - b0];
#if LDW_ABLATE_DECAY == 2   // (timing only: the distance without circ_len's division; right for positions within one turn only)
        const double dd = fabs(pt - pf), len = dd > 0.5 * g ? g - dd : dd;
#else
        const double len = circ_len(pt, pf, g);
#endif
        int bin = cuts_below(s_cuts, lo, hi, len);
        const int mb = mi_bucket(mi) >> A.mi_shift;
        const unsigned long long key = f64_key(mi);
        const bool outside = active && ((bin == lo && !(cut_under < len)) || (bin == hi && cut_top < len));
        if (outside) {   // (never in exact arithmetic)
            bin = cuts_below(s_cuts, 0, A.n_cut, len);
            atomicAdd(&A.hist[(size_t)bin * NB + mb], 1ull);
            max_to_global(&A.maxkey[bin], key);
            atomicAdd(&A.stat[2], 1ull);
        }
        bool todo = active && !outside;
        if (todo) {
            if (bin != cur_bin) {
                flush_max();
                cur_bin = bin, cur_key = key;
            } else if (key > cur_key)
                cur_key = key;
        }
        unsigned long long rem = __ballot(todo);
#if LDW_ABLATE_DECAY == 1   // (timing only, empty histogram: no counter is touched)
        rem = 0;
#endif
        if (lds) {
            if (rem) {
                const unsigned k = (unsigned)((bin - lo) * NB + mb);
                const int first = __ffsll((long long)rem) - 1;
                const unsigned k0 = (unsigned)__shfl((int)k, first);
                const unsigned long long same = __ballot(todo && k == k0);
                if (lane == first) atomicAdd(&s_cnt[k0], (uint32_t)__popcll(same));
                else if (todo && k != k0) atomicAdd(&s_cnt[k], 1u);
            }
        } else {
            const unsigned k = (unsigned)(bin * NB + mb);
            while (rem) {
                const int first = __ffsll((long long)rem) - 1;
                const unsigned k0 = (unsigned)__shfl((int)k, first);
                const unsigned long long same = __ballot(todo && k == k0);
                if (lane == first) atomicAdd(&A.hist[k0], (unsigned long long)__popcll(same));
                if (k == k0) todo = false;
                rem &= ~same;
            }
        }
    };
    // DEC_U columns of a wave are loaded before the first is counted: one 512-byte load in flight per wave leaves the kernel waiting for memory
    for (int64_t bb = b0 + w; bb < b1; bb += DEC_WAVES * DEC_U) {
        double v[DEC_U];
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            const int64_t b = bb + u * DEC_WAVES;
            v[u] = (b < b1 && row_ok && (A.diag ? a > b : a != b)) ? A.MI[a + b * A.nf] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < DEC_U; ++u)
            if (bb + u * DEC_WAVES < b1) count(bb + u * DEC_WAVES, v[u]);
    }
    flush_max();
    if (!lds) return;
    __syncthreads();
    unsigned long long *dst = A.hist + (size_t)lo * NB;   // the window's counters are contiguous in the output
    for (int i = tid; i < W * NB; i += DEC_THREADS) {
        const uint32_t v = s_cnt[i];
        if (v) atomicAdd(&dst[i], (unsigned long long)v);
    }
    if (tid < W && s_max[tid]) max_to_global(&A.maxkey[lo + tid], s_max[tid]);
}

// One profile: the device-side results and what every block's launch shares
struct DecayRun {
    DevBuf hist, maxkey, cuts, stat;
    int n_cut = 0, mi_shift = 0, NB = NBINS;
    size_t hist_bytes() const { return (size_t)(n_cut + 1) * NB * 8; }
};

static int decay_check(const double *cuts, int32_t n_cut, int32_t mi_shift, const char *who) {
    LDW_REQUIRE(n_cut >= 0 && n_cut <= DEC_MAX_CUTS, LDW_ERR_ARG, "%s: n_cut %d outside 0..%d", who, (int)n_cut, DEC_MAX_CUTS);
    LDW_REQUIRE(mi_shift >= 0 && mi_shift <= 6, LDW_ERR_ARG, "%s: mi_shift %d outside 0..6", who, (int)mi_shift);
    LDW_REQUIRE(n_cut == 0 || cuts, LDW_ERR_ARG, "%s: null cuts", who);
    for (int32_t k = 0; k < n_cut; ++k) {
        LDW_REQUIRE(std::isfinite(cuts[k]) && cuts[k] >= 0, LDW_ERR_ARG, "%s: cut %d is not a finite non-negative number", who, (int)k);
        LDW_REQUIRE(k == 0 || cuts[k] > cuts[k - 1], LDW_ERR_ARG, "%s: the cuts do not ascend strictly at %d", who, (int)k);
    }
    return LDW_OK;
}

static int decay_begin(ldw_ctx *c, DecayRun &R, const double *cuts, int32_t n_cut, int32_t mi_shift) {
    R.n_cut = n_cut, R.mi_shift = mi_shift, R.NB = NBINS >> mi_shift;
    if (int rc = R.hist.reserve(R.hist_bytes())) return rc;
    if (int rc = R.maxkey.reserve((size_t)(n_cut + 1) * 8)) return rc;
    if (int rc = R.stat.reserve(32)) return rc;
    if (int rc = upload(c, R.cuts, cuts, (size_t)n_cut)) return rc;
    LDW_HIP(hipMemsetAsync(R.hist.p, 0, R.hist_bytes(), c->stream));
    LDW_HIP(hipMemsetAsync(R.maxkey.p, 0, (size_t)(n_cut + 1) * 8, c->stream));
    LDW_HIP(hipMemsetAsync(R.stat.p, 0, 32, c->stream));
    return LDW_OK;
}

static int decay_launch(ldw_ctx *c, const DecayRun &R, const double *MI, int64_t nf, int64_t nt, const int32_t *pos_f, const int32_t *idx_f, const int32_t *pos_t,
                        const int32_t *idx_t, double g, int diag, int route) {
    DecayArgs A;
    A.MI = MI, A.nf = nf, A.nt = nt;
    A.pos_f = pos_f, A.pos_t = pos_t, A.idx_f = idx_f, A.idx_t = idx_t;
    A.g = g, A.diag = diag;
    A.cuts = R.cuts.as<double>(), A.n_cut = R.n_cut, A.mi_shift = R.mi_shift, A.route = route;
    A.hist = R.hist.as<unsigned long long>(), A.maxkey = R.maxkey.as<unsigned long long>(), A.stat = R.stat.as<unsigned long long>();
    const dim3 grid((unsigned)((nf + DEC_ROWS - 1) / DEC_ROWS), (unsigned)((nt + DEC_C - 1) / DEC_C));
    hipLaunchKernelGGL(k_decay_hist, grid, dim3(DEC_THREADS), 0, c->stream, A);
    LDW_HIP(hipGetLastError());
    return LDW_OK;
}

// the results to the host; stat_out[4] as DecayArgs::stat
static int decay_end(ldw_ctx *c, const DecayRun &R, uint64_t *hist_out, double *max_out, unsigned long long stat_out[4]) {
    std::vector<unsigned long long> keys((size_t)R.n_cut + 1);
    LDW_HIP(hipMemcpyAsync(hist_out, R.hist.p, R.hist_bytes(), hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemcpyAsync(keys.data(), R.maxkey.p, keys.size() * 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemcpyAsync(stat_out, R.stat.p, 32, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    if (max_out)
        for (size_t k = 0; k < keys.size(); ++k) max_out[k] = keys[k] ? key_f64(keys[k]) : std::nan("");
    return LDW_OK;
}

static int64_t decay_pairs(int64_t nf, int64_t nt, bool diag) { return diag ? nf * (nf - 1) / 2 : nf * nt - std::min(nf, nt); }

// ---- the block walk of ldw_mi_profile and ldw_mi_snp_summary (ldw_internal.h) ----
int pair_blocks_check(ldw_ctx *c, const char *who, const int32_t *blocks, int64_t nblocks, int quirk_mode, bool outputs_ok, const std::function<int()> &own_check) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(blocks && nblocks > 0 && outputs_ok, LDW_ERR_ARG, "%s: bad argument", who);
    LDW_REQUIRE(quirk_mode == LDW_QUIRK_REFERENCE || quirk_mode == LDW_QUIRK_INTENDED, LDW_ERR_ARG, "%s: bad quirk mode", who);
    LDW_REQUIRE(have_alignment(c) && c->wts.have_weights && c->meta.have_meta, LDW_ERR_STATE, "%s needs the alignment, the weights and the SNP meta data to be set first", who);
    if (int rc = own_check()) return rc;   // (the caller's own arguments are judged before the blocks, as ldw_mi_profile always did)
    for (int64_t b = 0; b < nblocks; ++b) {
        const int32_t fs = blocks[b * 4 + 0], fe = blocks[b * 4 + 1], ts = blocks[b * 4 + 2], te = blocks[b * 4 + 3];
        LDW_REQUIRE(fs >= 1 && fs <= fe && fe <= c->L && ts >= 1 && ts <= te && te <= c->L, LDW_ERR_ARG, "%s: block %lld (%d..%d x %d..%d) outside 1..%lld", who, (long long)b,
                    fs, fe, ts, te, (long long)c->L);
        LDW_REQUIRE((fs == ts && fe == te) || fe < ts || te < fs, LDW_ERR_ARG, "%s: the ranges of block %lld (%d..%d x %d..%d) overlap without being equal", who, (long long)b,
                    fs, fe, ts, te);
    }
    return LDW_OK;
}

int pair_blocks_walk(ldw_ctx *c, const int32_t *blocks, int64_t nblocks, int quirk_mode, PairBlockWalk &W, const std::function<int(int64_t, int64_t, bool)> &consumer) {
    std::vector<int32_t> fi, ti;
    for (int64_t b = 0; b < nblocks; ++b) {
        const int32_t fs = blocks[b * 4 + 0], fe = blocks[b * 4 + 1], ts = blocks[b * 4 + 2], te = blocks[b * 4 + 3];
        const int64_t nf = fe - fs + 1, nt = te - ts + 1;
        const bool diag = fs == ts && fe == te;
        fi.resize((size_t)nf), ti.resize((size_t)nt);
        for (int64_t k = 0; k < nf; ++k) fi[(size_t)k] = fs - 1 + (int32_t)k;
        for (int64_t k = 0; k < nt; ++k) ti[(size_t)k] = ts - 1 + (int32_t)k;
        if (int rc = block_mi_dense(c, fi.data(), nf, ti.data(), nt, quirk_mode)) return rc;   // (leaves the block's index lists in ctx->idx_f / idx_t)
        LDW_HIP(hipEventRecord(c->ev[3], c->stream));
        if (int rc = consumer(nf, nt, diag)) return rc;
        LDW_HIP(hipEventRecord(c->ev[4], c->stream));
        LDW_HIP(hipStreamSynchronize(c->stream));   // (the next block's staging overwrites the lists and the events)
        float t01 = 0, t12 = 0, t34 = 0;
        LDW_HIP(hipEventElapsedTime(&t01, c->ev[0], c->ev[1]));
        LDW_HIP(hipEventElapsedTime(&t12, c->ev[1], c->ev[2]));
        LDW_HIP(hipEventElapsedTime(&t34, c->ev[3], c->ev[4]));
        W.ms_mi += (double)t01 + t12, W.ms_consumer += t34;
        W.npairs += decay_pairs(nf, nt, diag);
    }
    return LDW_OK;
}

}  // namespace ldw

extern "C" {

int ldw_mi_profile(ldw_ctx *c, const int32_t *blocks, int64_t nblocks, int quirk_mode, const double *cuts, int32_t n_cut, int32_t mi_shift, uint64_t *hist_out,
                   double *max_out, int64_t *npairs_out) {
    if (int rc = pair_blocks_check(c, "ldw_mi_profile", blocks, nblocks, quirk_mode, hist_out && npairs_out,
                                   [&] { return decay_check(cuts, n_cut, mi_shift, "ldw_mi_profile"); }))
        return rc;
    DecayRun R;
    if (int rc = decay_begin(c, R, cuts, n_cut, mi_shift)) return rc;
    PairBlockWalk W;
    if (int rc = pair_blocks_walk(c, blocks, nblocks, quirk_mode, W, [&](int64_t nf, int64_t nt, bool diag) {
            return decay_launch(c, R, c->MIblk.as<double>(), nf, nt, c->meta.POS.as<int32_t>(), c->idx_f.as<int32_t>(), c->meta.POS.as<int32_t>(), c->idx_t.as<int32_t>(),
                                c->meta.g, diag ? 1 : 0, 0);
        }))
        return rc;
    unsigned long long st[4];
    if (int rc = decay_end(c, R, hist_out, max_out, st)) return rc;
    *npairs_out = W.npairs;
    c->decay_stat[0] = (int64_t)st[0], c->decay_stat[1] = (int64_t)st[1], c->decay_stat[2] = (int64_t)st[2], c->decay_stat[3] = nblocks;
    c->last_ms[0] = W.ms_mi, c->last_ms[1] = W.ms_consumer, c->last_ms[2] = 0, c->last_ms[3] = W.ms_mi + W.ms_consumer;
    return LDW_OK;
}

int ldw_decay_report(ldw_ctx *c, int64_t out[4]) {
    LDW_REQUIRE(c && out, LDW_ERR_ARG, "ldw_decay_report: null argument");
    for (int k = 0; k < 4; ++k) out[k] = c->decay_stat[k];
    return LDW_OK;
}

int ldw_debug_profile_hist(ldw_ctx *c, const double *mi, int64_t nf, int64_t nt, const int32_t *pos_f, const int32_t *pos_t, double g, int diag, const double *cuts,
                           int32_t n_cut, int32_t mi_shift, int route, uint64_t *hist_out, double *max_out, int64_t *npairs_out, int64_t *stats_out) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(mi && pos_f && pos_t && hist_out && npairs_out, LDW_ERR_ARG, "ldw_debug_profile_hist: null argument");
    LDW_REQUIRE(nf >= 1 && nt >= 1 && nf <= 1000000 && nt <= 1000000, LDW_ERR_ARG, "ldw_debug_profile_hist: nf, nt outside 1..1 000 000");
    LDW_REQUIRE(diag == 0 || (diag == 1 && nf == nt), LDW_ERR_ARG, "ldw_debug_profile_hist: diag is 0 or 1, and a diagonal block is square");
    LDW_REQUIRE(std::isfinite(g) && g > 0, LDW_ERR_ARG, "ldw_debug_profile_hist: g must be positive");
    LDW_REQUIRE(route >= 0 && route <= 2, LDW_ERR_ARG, "ldw_debug_profile_hist: route outside 0..2");
    if (int rc = decay_check(cuts, n_cut, mi_shift, "ldw_debug_profile_hist")) return rc;
    if (int rc = join_prepare(c)) return rc;
    DecayRun R;
    DevBuf d_mi, d_pf, d_pt;
    if (int rc = decay_begin(c, R, cuts, n_cut, mi_shift)) return rc;
    if (int rc = upload(c, d_mi, mi, (size_t)(nf * nt))) return rc;
    if (int rc = upload(c, d_pf, pos_f, (size_t)nf)) return rc;
    if (int rc = upload(c, d_pt, pos_t, (size_t)nt)) return rc;
    if (int rc = decay_launch(c, R, d_mi.as<double>(), nf, nt, d_pf.as<int32_t>(), nullptr, d_pt.as<int32_t>(), nullptr, g, diag, route)) return rc;
    unsigned long long st[4];
    if (int rc = decay_end(c, R, hist_out, max_out, st)) return rc;
    LDW_REQUIRE(st[3] == 0, LDW_ERR_ARG, "ldw_debug_profile_hist: route 1, but the window of %llu patches does not fit %d counters", st[3], DEC_LDS_CNT);
    *npairs_out = decay_pairs(nf, nt, diag != 0);
    if (stats_out)
        for (int k = 0; k < 3; ++k) stats_out[k] = (int64_t)st[k];
    return LDW_OK;
}

}  // extern "C"
