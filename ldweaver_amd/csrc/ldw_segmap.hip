// Segment x segment map over EVERY SNP pair of a block list (ldweaver_amd.h 24): seg[L] labels the SNPs (genes, equal stretches of the
// genome, anything), and the cell (min(seg[A], seg[B]), max(seg[A], seg[B])) of the pair (A, B) takes the pair's value v = mi, or mi - w[A] w[B]
// (ldw_score.h).  Two walks over the blocks and pair set of ldw_mi_profile, each one launch per block behind the block's epilogue, each reading the dense
// block of the plain path (block_mi_dense -> ctx->MIblk, column-major) once:
//   k_segment<false>  per cell the number of pairs, the pairs with v >= thr, the sum of q(v) in two words (ldw_segmap.h) and the largest value (f64_key order);
//   k_segment<true>   per cell the smallest packed pair (min(A, B) << 32 | max(A, B)) whose value has the key of the caller's max_in.
// Every output is an integer add, a maximum of an order-preserving 64-bit key or a 64-bit integer minimum: no result depends on the order of evaluation,
// and there is no floating-point atomic.
//
// Both keep the patch shape of k_decay_hist and k_snp_summary: a workgroup of four waves takes 64 rows (a_loc, the lanes) x SM_C columns (b_loc; wave w takes
// the SM_WC contiguous columns w * SM_WC ..., eight loads in flight).  The class of a pair is circ_len per pair, never a bound of the patch.  The segment
// ids of a patch's rows and of its columns are cut into runs (a run ends where the id differs from the neighbour's; two runs may carry one id), and the
// patch takes one of two routes:
//   (1) at most SM_RR row runs and SM_CR column runs: a window of SM_RR x SM_CR cells in LDS.  The column run of a wave's column is the same in every lane,
//       so a lane accumulates in registers while the run lasts; where it changes, the lanes that share a row run are summed across the wave and lane 0 adds
//       the totals to the window cell.  At the end every non-empty window cell makes one global add or maximum per quantity.  The best kernel keeps the
//       window's max_in keys in LDS instead, the key of the lane's current cell in a register, and touches global memory on a match only.
//   (2) else: per column the lanes that share a cell are combined in a readfirstlane / ballot loop (k_decay_hist's route B) and the first of them adds to
//       the global cell; the best kernel reads max_in's key of its cell per pair.
// Both routes give the same integers.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ldw_internal.h"
#include "ldw_dev.h"
#include "ldw_score.h"
#include "ldw_segmap.h"
#include "ldw_work.h"

using namespace ldw;

namespace ldw {

#ifndef LDW_ABLATE_SEGMAP
#define LDW_ABLATE_SEGMAP 0   // measurement builds (make VARIANT=.. EXTRA_DEFS=-DLDW_ABLATE_SEGMAP=n): 1 = the map accumulates nothing (loads, class and value only); DESIGN.md 35
#endif
constexpr int SM_ROWS = 64;          // rows of a patch: the lanes of a wave
constexpr int SM_C = 256;            // columns of a patch
constexpr int SM_THREADS = 256;
constexpr int SM_WAVES = SM_THREADS / 64;
constexpr int SM_WC = SM_C / SM_WAVES;   // contiguous columns of a wave
constexpr int SM_U = 8;              // columns a wave has in flight
constexpr int SM_RR = 8;             // row runs of route 1's window
constexpr int SM_CR = 16;            // column runs of route 1's window
constexpr int SM_CELLS = SM_RR * SM_CR;
constexpr int SM_NSTAT = 8;          // [0] patches visited, [1] patches on route 2, [2] values q refused, [3] NaN values, [4] patches route 1 refused, [5] pairs that took part
constexpr int SM_MAX_S = 8192;
static_assert(SM_C == SM_THREADS, "every thread fetches the position, the weight and the segment of one column of the patch");
static_assert(SM_WC % SM_U == 0, "a wave's columns are whole batches");
static_assert(SM_RR >= 4 && SM_CR >= 8 && SM_CELLS < SM_ROWS * SM_C && SM_CELLS <= SM_THREADS, "the window: at least 4 x 8 runs, one thread per cell");

struct SegSide {
    const int32_t *pos, *idx;       // the position, the segment and the weight of local index i are those of idx[i] (null: i itself)
    const int32_t *seg;
    const int32_t *id;              // the global SNP of local index i (the best kernel alone reads it)
    const double *w;                // null: the value is the MI itself
};

struct SegArgs {
    const double *MI;               // [nf * nt] column-major: the pair (a_loc, b_loc) at a_loc + b_loc * nf
    int64_t nf, nt;
    SegSide F, T;                   // the from side (rows) and the to side (columns)
    double g, sr_dist, thr;
    int diag;                       // 1: pairs a_loc > b_loc; 0: pairs a_loc != b_loc
    int cls_mask;                   // 1: circ_len <= sr_dist, 2: beyond, 3: both (no distance is computed)
    int route;                      // 0: the patch chooses; 1: runs or refuse; 2: general
    int S;
    unsigned long long *n, *nge, *lo, *hi, *key;   // map: [S * S] each
    const unsigned long long *keyin;               // best: the keys of max_in, 0 = NaN
    unsigned long long *pair;                      // best: the smallest matching packed pair so far, all-ones = none
    unsigned long long *stat;       // [SM_NSTAT]
};

__device__ __forceinline__ void seg_max(unsigned long long *p, unsigned long long key) {
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key) atomicMax(p, key);
}
__device__ __forceinline__ unsigned long long lanes_up_to(int lane) { return (2ull << lane) - 1ull; }   // (lane 63: 2 << 63 wraps to 0, all ones)
__device__ __forceinline__ int seg_cell(int sa, int sb, int S) { return (sa < sb ? sa : sb) * S + (sa < sb ? sb : sa); }

// No second launch bound: the compiler takes 103 (map) and 98 (best) registers without scratch, four waves per SIMD; 9 856 and 10 880 bytes of LDS
template <bool BEST>
__global__ __launch_bounds__(SM_THREADS) void k_segment(SegArgs A) {
    __shared__ unsigned long long s_lo[SM_CELLS], s_hi[SM_CELLS], s_key[SM_CELLS];   // the window: the two sum words and the key of the maximum (best: the keys of max_in)
    __shared__ uint32_t s_n[SM_CELLS], s_g[SM_CELLS];                                 // its pairs and its pairs at or above the threshold
    __shared__ int s_gc[SM_CELLS];           // the global cell of a window cell, -1: none
    __shared__ unsigned long long s_wb[SM_WAVES];   // the run starts among a wave's columns
    __shared__ double s_wt[SM_C];            // the weights of the patch's columns
    __shared__ int s_pt[SM_C], s_cs[SM_C], s_cr[SM_C], s_id[SM_C];   // their positions, segments, run slots and global SNPs
    __shared__ int s_rseg[SM_RR], s_cseg[SM_CR];   // the segment of every run
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t a0 = (int64_t)blockIdx.x * SM_ROWS, b0 = (int64_t)blockIdx.y * SM_C;
    const int64_t a1 = a0 + SM_ROWS < A.nf ? a0 + SM_ROWS : A.nf, b1 = b0 + SM_C < A.nt ? b0 + SM_C : A.nt;
    if (A.diag && a1 - 1 <= b0) return;   // no pair a_loc > b_loc in the patch
    const bool has_w = A.F.w != nullptr;
    const int64_t a = a0 + lane;
    const bool row_ok = a < a1;
    const int64_t ia = row_ok ? (A.F.idx ? A.F.idx[a] : a) : 0;
    const double pf = row_ok ? (double)A.F.pos[ia] : 0.0, wa = row_ok && has_w ? A.F.w[ia] : 0.0;
    const int sa = row_ok ? A.F.seg[ia] : -1;
    const unsigned id_a = BEST && row_ok ? (unsigned)(A.F.id ? A.F.id[a] : (int)a) : 0u;
    const bool col_ok = b0 + tid < b1;
    int cs = -1;
    if (col_ok) {
        const int64_t ib = A.T.idx ? A.T.idx[b0 + tid] : b0 + tid;
        cs = A.T.seg[ib];
        s_pt[tid] = A.T.pos[ib], s_wt[tid] = has_w ? A.T.w[ib] : 0.0;
        if (BEST) s_id[tid] = A.T.id ? A.T.id[b0 + tid] : (int)(b0 + tid);
    }
    s_cs[tid] = cs;
    // the row runs (every wave holds the same 64 rows): a run starts where the id differs from the row above
    const int sa_up = __shfl_up(sa, 1);
    const bool rb = lane > 0 && row_ok && sa != sa_up;
    const unsigned long long rbal = __ballot(rb);
    const int rrun = __popcll(rbal & lanes_up_to(lane)), nrr = __popcll(rbal) + 1;
    __syncthreads();
    // the column runs, over the four waves
    const bool cb = tid > 0 && col_ok && cs != s_cs[tid - 1];
    const unsigned long long cbal = __ballot(cb);
    if (lane == 0) s_wb[w] = cbal;
    __syncthreads();
    int before = 0, ncr = 1;
#pragma unroll
    for (int v = 0; v < SM_WAVES; ++v) {
        const int p = __popcll(s_wb[v]);
        ncr += p, before += v < w ? p : 0;
    }
    const int crun = before + __popcll(cbal & lanes_up_to(lane));
    s_cr[tid] = crun;
    const bool fits = nrr <= SM_RR && ncr <= SM_CR;
    if (A.route == 1 && !fits) {
        if (tid == 0) atomicAdd(&A.stat[4], 1ull);
        return;
    }
    const bool runs = fits && A.route != 2;
    if (tid == 0) {
        atomicAdd(&A.stat[0], 1ull);
        if (!runs) atomicAdd(&A.stat[1], 1ull);
    }
    if (runs) {
        if (w == 0 && (lane == 0 || rb)) s_rseg[rrun] = sa;
        if (tid == 0 || cb) s_cseg[crun] = cs;
        __syncthreads();
        if (tid < SM_CELLS) {
            const int r = tid / SM_CR, cc = tid % SM_CR;
            int gc = -1;
            if (r < nrr && cc < ncr && s_rseg[r] >= 0 && s_cseg[cc] >= 0) gc = seg_cell(s_rseg[r], s_cseg[cc], A.S);
            s_gc[tid] = gc;
            s_n[tid] = s_g[tid] = 0, s_lo[tid] = s_hi[tid] = 0;
            s_key[tid] = BEST && gc >= 0 ? A.keyin[gc] : 0ull;
        }
    }
    __syncthreads();
    uint32_t n_ = 0, g_ = 0;              // of the lane's row over the columns of the current column run
    unsigned long long lo_ = 0, key_ = 0;
    long long hi_ = 0;
    uint32_t n_ref = 0, n_nan = 0, n_in = 0;   // of the lane: values q refused, NaN values, pairs that took part
    int cur = -1;                         // the current column run
    unsigned long long kin = 0;           // best: the key of max_in of the lane's current cell
    auto flush = [&]() {                  // the lanes' sums to the window's cells (cur, row run)
        if (BEST || cur < 0 || !__ballot(n_ != 0)) return;
        for (int r = 0; r < nrr; ++r) {
            const bool mine = rrun == r;
            uint32_t tn = mine ? n_ : 0, tg = mine ? g_ : 0;
            unsigned long long tl = mine ? lo_ : 0, tk = mine ? key_ : 0;
            long long th = mine ? hi_ : 0;
#pragma unroll
            for (int o = 32; o; o >>= 1) {
                tn += __shfl_xor(tn, o), tg += __shfl_xor(tg, o), tl += __shfl_xor(tl, o), th += __shfl_xor(th, o);
                const unsigned long long ok = __shfl_xor(tk, o);
                tk = ok > tk ? ok : tk;
            }
            if (lane == 0 && tn) {
                const int k = r * SM_CR + cur;
                atomicAdd(&s_n[k], tn);
                if (tg) atomicAdd(&s_g[k], tg);
                if (tl) atomicAdd(&s_lo[k], tl);
                if (th) atomicAdd(&s_hi[k], (unsigned long long)th);
                if (tk) atomicMax(&s_key[k], tk);
            }
        }
        n_ = g_ = 0, lo_ = key_ = 0, hi_ = 0;
    };
    const int64_t wb0 = b0 + (int64_t)w * SM_WC;
    const int64_t wb1 = wb0 + SM_WC < b1 ? wb0 + SM_WC : b1;
    for (int64_t bb = wb0; bb < wb1; bb += SM_U) {
        if (A.diag && a1 - 1 <= bb) break;   // no pair a_loc > b_loc in these columns or in later ones
        double mv[SM_U];
#pragma unroll
        for (int u = 0; u < SM_U; ++u) {
            const int64_t b = bb + u;
            mv[u] = (b < b1 && row_ok && (A.diag ? a > b : a != b)) ? A.MI[a + b * A.nf] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < SM_U; ++u) {
            const int64_t b = bb + u;
            const int j = (int)(b - b0);   // (j < SM_C: within the LDS arrays also past b1, where no lane is active)
            const int sb = s_cs[j];
            bool active = b < b1 && row_ok && (A.diag ? a > b : a != b) && sa >= 0 && sb >= 0;
            if (A.cls_mask != 3) active = active && ((circ_len((double)s_pt[j], pf, A.g) <= A.sr_dist ? 1 : 2) & A.cls_mask) != 0;
            const double v = has_w ? pair_score(mv[u], wa, s_wt[j]) : mv[u];
            const bool valid = active && v == v;
            const unsigned long long key = valid ? f64_key(v) : 0ull;   // (0: no number's key)
            n_in += active, n_nan += active && !valid;
            if (runs) {
                const int cr = __builtin_amdgcn_readfirstlane(s_cr[j]);
                if (cr != cur) {
                    flush();
                    cur = cr;
                    if (BEST) kin = s_key[rrun * SM_CR + cr];
                }
            }
            if constexpr (BEST) {
                const unsigned id_b = (unsigned)s_id[j];
                const unsigned long long packed = ((unsigned long long)(id_a < id_b ? id_a : id_b) << 32) | (unsigned long long)(id_a < id_b ? id_b : id_a);
                if (runs) {
                    if (valid && key == kin) atomicMin(&A.pair[s_gc[rrun * SM_CR + cur]], packed);
                } else if (valid) {
                    const int cell = seg_cell(sa, sb, A.S);
                    if (key == A.keyin[cell]) atomicMin(&A.pair[cell], packed);
                }
            } else {
                bool ref;
                long long ql, qh;
                segmap_split(segmap_q(v, &ref), (int64_t *)&ql, (int64_t *)&qh);
                const bool ge = active && v >= A.thr;   // (an fp64 comparison: false for a NaN value and for a NaN threshold)
                n_ref += active && ref;
#if LDW_ABLATE_SEGMAP != 1
                if (runs) {
                    n_ += active, g_ += ge;
                    lo_ += active ? (unsigned long long)ql : 0ull, hi_ += active ? qh : 0ll;
                    key_ = key > key_ ? key : key_;
                } else {
                    const int cell = active ? seg_cell(sa, sb, A.S) : -1;
                    bool todo = active;
                    unsigned long long rem = __ballot(todo);
                    while (rem) {   // the lanes that share the first remaining lane's cell are added as one
                        const int first = __ffsll((long long)rem) - 1;
                        const int c0 = __shfl(cell, first);
                        const bool mine = todo && cell == c0;
                        const unsigned long long same = __ballot(mine);
                        const int cnt = __popcll(same), cge = __popcll(__ballot(mine && ge));
                        unsigned long long tl = mine ? (unsigned long long)ql : 0ull, tk = mine ? key : 0ull;
                        long long th = mine ? qh : 0ll;
                        if (cnt > 1) {
#pragma unroll
                            for (int o = 32; o; o >>= 1) {
                                tl += __shfl_xor(tl, o), th += __shfl_xor(th, o);
                                const unsigned long long ok = __shfl_xor(tk, o);
                                tk = ok > tk ? ok : tk;
                            }
                        }
                        if (lane == first) {
                            atomicAdd(&A.n[c0], (unsigned long long)cnt);
                            if (cge) atomicAdd(&A.nge[c0], (unsigned long long)cge);
                            if (tl) atomicAdd(&A.lo[c0], tl);
                            if (th) atomicAdd(&A.hi[c0], (unsigned long long)th);
                            if (tk) seg_max(&A.key[c0], tk);
                        }
                        todo = todo && !mine;
                        rem &= ~same;
                    }
                }
#endif
            }
        }
    }
    flush();
    for (int o = 32; o; o >>= 1) n_ref += __shfl_xor(n_ref, o), n_nan += __shfl_xor(n_nan, o), n_in += __shfl_xor(n_in, o);
    if (lane == 0) {
        if (n_ref) atomicAdd(&A.stat[2], (unsigned long long)n_ref);
        if (n_nan) atomicAdd(&A.stat[3], (unsigned long long)n_nan);
        if (n_in) atomicAdd(&A.stat[5], (unsigned long long)n_in);
    }
    if (BEST || !runs) return;
    __syncthreads();
    if (tid < SM_CELLS && s_gc[tid] >= 0 && s_n[tid]) {   // one global operation per quantity of a window cell that is not zero
        const int gc = s_gc[tid];
        atomicAdd(&A.n[gc], (unsigned long long)s_n[tid]);
        if (s_g[tid]) atomicAdd(&A.nge[gc], (unsigned long long)s_g[tid]);
        if (s_lo[tid]) atomicAdd(&A.lo[gc], s_lo[tid]);
        if (s_hi[tid]) atomicAdd(&A.hi[gc], s_hi[tid]);
        if (s_key[tid]) seg_max(&A.key[gc], s_key[tid]);
    }
}

// One walk: the per-SNP vectors staged once, the device-side results and counters, all carved from one working buffer
struct SegRun {
    DevBuf work;
    Carve cv;
    unsigned long long *n = nullptr, *nge = nullptr, *lo = nullptr, *hi = nullptr, *key = nullptr, *keyin = nullptr, *pair = nullptr, *stat = nullptr;
    int32_t *seg_f = nullptr, *seg_t = nullptr;
    double *w_f = nullptr, *w_t = nullptr;
    std::vector<unsigned long long> h_keyin;   // (outlives its copy)
    int64_t cells = 0;
    int S = 0;
    bool best = false, has_w = false;
    double thr = 0;
};

static int segmap_check(const int32_t *seg, int64_t n, const char *sname, int32_t S, double sr_dist, int cls_mask, const double *w, const char *wname, const char *who) {
    LDW_REQUIRE(S >= 1 && S <= SM_MAX_S, LDW_ERR_ARG, "%s: S %d outside 1..%d", who, (int)S, SM_MAX_S);
    LDW_REQUIRE(seg, LDW_ERR_ARG, "%s: null %s", who, sname);
    for (int64_t i = 0; i < n; ++i) LDW_REQUIRE(seg[i] >= -1 && seg[i] < S, LDW_ERR_ARG, "%s: %s[%lld] = %d outside -1..%d", who, sname, (long long)i, (int)seg[i], (int)S - 1);
    LDW_REQUIRE(!std::isnan(sr_dist) && sr_dist >= 0, LDW_ERR_ARG, "%s: sr_dist must be a non-negative number (+inf allowed)", who);
    LDW_REQUIRE(cls_mask >= 1 && cls_mask <= 3, LDW_ERR_ARG, "%s: cls_mask %d outside 1..3", who, cls_mask);
    if (w)
        for (int64_t i = 0; i < n; ++i) LDW_REQUIRE(std::isfinite(w[i]), LDW_ERR_ARG, "%s: %s[%lld] is not finite", who, wname, (long long)i);
    return LDW_OK;
}

// a block list of 2^39 pairs or more could overflow a cell's sum words
static int segmap_size(const int32_t *blocks, int64_t nblocks, const char *who) {
    int64_t total = 0;
    for (int64_t b = 0; b < nblocks; ++b) {
        const int64_t nf = blocks[b * 4 + 1] - blocks[b * 4 + 0] + 1, nt = blocks[b * 4 + 3] - blocks[b * 4 + 2] + 1;
        const bool diag = blocks[b * 4 + 0] == blocks[b * 4 + 2] && blocks[b * 4 + 1] == blocks[b * 4 + 3];
        total += diag ? nf * (nf - 1) / 2 : nf * nt - std::min(nf, nt);
        LDW_REQUIRE(total < (int64_t(1) << 39), LDW_ERR_SIZE, "%s: the blocks hold 2^39 pairs or more: a cell's sum could overflow", who);
    }
    return LDW_OK;
}

static int seg_begin(ldw_ctx *c, SegRun &R, int32_t S, const int32_t *seg_f, const int32_t *seg_t, const double *w_f, const double *w_t, int64_t lenF, int64_t lenT,
                     const double *max_in) {
    R.S = S, R.cells = (int64_t)S * S, R.best = max_in != nullptr, R.has_w = w_f != nullptr;
    const bool shared = seg_t == nullptr;   // both sides read the from side's vectors (the SNPs of an alignment)
    Carve &cv = R.cv;
    auto n = cv.take<unsigned long long>(R.best ? 0 : R.cells), nge = cv.take<unsigned long long>(R.best ? 0 : R.cells);
    auto lo = cv.take<unsigned long long>(R.best ? 0 : R.cells), hi = cv.take<unsigned long long>(R.best ? 0 : R.cells);
    auto key = cv.take<unsigned long long>(R.best ? 0 : R.cells), stat = cv.take<unsigned long long>(SM_NSTAT);
    auto keyin = cv.take<unsigned long long>(R.best ? R.cells : 0), pair = cv.take<unsigned long long>(R.best ? R.cells : 0);
    auto sf = cv.take<int32_t>(lenF), st = cv.take<int32_t>(shared ? 0 : lenT);
    auto wf = cv.take<double>(R.has_w ? lenF : 0), wt = cv.take<double>(R.has_w && !shared ? lenT : 0);
    if (int rc = cv.reserve(R.work)) return rc;
    R.n = n, R.nge = nge, R.lo = lo, R.hi = hi, R.key = key, R.stat = stat, R.keyin = keyin, R.pair = pair;
    R.seg_f = sf, R.seg_t = shared ? (int32_t *)sf : (int32_t *)st;
    R.w_f = R.has_w ? (double *)wf : nullptr, R.w_t = R.has_w ? (shared ? (double *)wf : (double *)wt) : nullptr;
    const Carve::Range zero = cv.cover(n, nge, lo, hi, key, stat);
    LDW_HIP(hipMemsetAsync(zero.p, 0, zero.bytes, c->stream));
    if (R.best) {
        R.h_keyin.resize((size_t)R.cells);
        for (int64_t k = 0; k < R.cells; ++k) R.h_keyin[(size_t)k] = std::isnan(max_in[k]) ? 0ull : (unsigned long long)f64_key(max_in[k]);   // 0 for NaN: no value has that key
        LDW_HIP(hipMemcpyAsync(R.keyin, R.h_keyin.data(), (size_t)R.cells * 8, hipMemcpyHostToDevice, c->stream));
        LDW_HIP(hipMemsetAsync(R.pair, 0xFF, (size_t)R.cells * 8, c->stream));
    }
    LDW_HIP(hipMemcpyAsync(R.seg_f, seg_f, (size_t)lenF * 4, hipMemcpyHostToDevice, c->stream));
    if (!shared) LDW_HIP(hipMemcpyAsync(R.seg_t, seg_t, (size_t)lenT * 4, hipMemcpyHostToDevice, c->stream));
    if (R.has_w) {
        LDW_HIP(hipMemcpyAsync(R.w_f, w_f, (size_t)lenF * 8, hipMemcpyHostToDevice, c->stream));
        if (!shared) LDW_HIP(hipMemcpyAsync(R.w_t, w_t, (size_t)lenT * 8, hipMemcpyHostToDevice, c->stream));
    }
    return LDW_OK;
}

static int seg_launch(ldw_ctx *c, const SegRun &R, const double *MI, int64_t nf, int64_t nt, const int32_t *pos_f, const int32_t *idx_f, const int32_t *id_f,
                      const int32_t *pos_t, const int32_t *idx_t, const int32_t *id_t, double g, int diag, double sr_dist, int cls_mask, int route) {
    SegArgs A;
    A.MI = MI, A.nf = nf, A.nt = nt;
    A.F.pos = pos_f, A.F.idx = idx_f, A.F.id = id_f, A.F.seg = R.seg_f, A.F.w = R.w_f;
    A.T.pos = pos_t, A.T.idx = idx_t, A.T.id = id_t, A.T.seg = R.seg_t, A.T.w = R.w_t;
    A.g = g, A.sr_dist = sr_dist, A.thr = R.thr, A.diag = diag, A.cls_mask = cls_mask, A.route = route, A.S = R.S;
    A.n = R.n, A.nge = R.nge, A.lo = R.lo, A.hi = R.hi, A.key = R.key, A.keyin = R.keyin, A.pair = R.pair, A.stat = R.stat;
    const dim3 grid((unsigned)((nf + SM_ROWS - 1) / SM_ROWS), (unsigned)((nt + SM_C - 1) / SM_C));
    if (R.best) LDW_LAUNCH(k_segment<true>, grid, dim3(SM_THREADS), 0, c->stream, A);
    else LDW_LAUNCH(k_segment<false>, grid, dim3(SM_THREADS), 0, c->stream, A);
    return LDW_OK;
}

// the map's matrices and the counters to the host; the stream is synchronised
static int map_fetch(ldw_ctx *c, const SegRun &R, int64_t *n_out, int64_t *nge_out, int64_t *lo_out, int64_t *hi_out, double *max_out, unsigned long long st[SM_NSTAT]) {
    const size_t bytes = (size_t)R.cells * 8;
    std::vector<unsigned long long> keys;
    LDW_HIP(hipMemcpyAsync(n_out, R.n, bytes, hipMemcpyDeviceToHost, c->stream));
    if (nge_out) LDW_HIP(hipMemcpyAsync(nge_out, R.nge, bytes, hipMemcpyDeviceToHost, c->stream));
    if (lo_out) LDW_HIP(hipMemcpyAsync(lo_out, R.lo, bytes, hipMemcpyDeviceToHost, c->stream));
    if (hi_out) LDW_HIP(hipMemcpyAsync(hi_out, R.hi, bytes, hipMemcpyDeviceToHost, c->stream));
    if (max_out) {
        keys.resize((size_t)R.cells);
        LDW_HIP(hipMemcpyAsync(keys.data(), R.key, bytes, hipMemcpyDeviceToHost, c->stream));
    }
    LDW_HIP(hipMemcpyAsync(st, R.stat, SM_NSTAT * 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    if (max_out)
        for (size_t k = 0; k < keys.size(); ++k) max_out[k] = keys[k] ? key_f64(keys[k]) : std::nan("");   // (NaN also for a cell whose every value is NaN)
    return LDW_OK;
}

static int best_fetch(ldw_ctx *c, const SegRun &R, uint64_t *pair_out, unsigned long long st[SM_NSTAT]) {
    LDW_HIP(hipMemcpyAsync(pair_out, R.pair, (size_t)R.cells * 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemcpyAsync(st, R.stat, SM_NSTAT * 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    return LDW_OK;
}

static void seg_done(ldw_ctx *c, const unsigned long long st[SM_NSTAT], int64_t nblocks, const PairBlockWalk &W) {
    for (int k = 0; k < 4; ++k) c->segmap_stat[k] = (int64_t)st[k];
    c->segmap_stat[4] = nblocks;
    c->last_ms[0] = W.ms_mi, c->last_ms[1] = W.ms_consumer, c->last_ms[2] = 0, c->last_ms[3] = W.ms_mi + W.ms_consumer;
}

static int seg_walk(ldw_ctx *c, const SegRun &R, const int32_t *blocks, int64_t nblocks, int quirk_mode, double sr_dist, int cls_mask, PairBlockWalk &W) {
    return pair_blocks_walk(c, blocks, nblocks, quirk_mode, W, [&](int64_t nf, int64_t nt, bool diag) {
        return seg_launch(c, R, c->MIblk.as<double>(), nf, nt, c->meta.POS.as<int32_t>(), c->idx_f.as<int32_t>(), c->idx_f.as<int32_t>(), c->meta.POS.as<int32_t>(),
                          c->idx_t.as<int32_t>(), c->idx_t.as<int32_t>(), c->meta.g, diag ? 1 : 0, sr_dist, cls_mask, 0);
    });
}

// what both debug entries require of the caller-made block
static int seg_debug_check(const char *who, const void *mi, int64_t nf, int64_t nt, const void *pos_f, const void *pos_t, double g, int diag, int route, const int32_t *seg_f,
                           const int32_t *seg_t, int32_t S, double sr_dist, int cls_mask, const double *w_f, const double *w_t) {
    LDW_REQUIRE(mi && pos_f && pos_t, LDW_ERR_ARG, "%s: null argument", who);
    LDW_REQUIRE(nf >= 1 && nt >= 1 && nf <= 1000000 && nt <= 1000000, LDW_ERR_ARG, "%s: nf, nt outside 1..1 000 000", who);
    LDW_REQUIRE(diag == 0 || (diag == 1 && nf == nt), LDW_ERR_ARG, "%s: diag is 0 or 1, and a diagonal block is square", who);
    LDW_REQUIRE(std::isfinite(g) && g > 0, LDW_ERR_ARG, "%s: g must be positive", who);
    LDW_REQUIRE(route >= 0 && route <= 2, LDW_ERR_ARG, "%s: route outside 0..2", who);
    LDW_REQUIRE((w_f != nullptr) == (w_t != nullptr), LDW_ERR_ARG, "%s: w_f and w_t are given both or neither", who);
    if (int rc = segmap_check(seg_f, nf, "seg_f", S, sr_dist, cls_mask, w_f, "w_f", who)) return rc;
    return segmap_check(seg_t, nt, "seg_t", S, sr_dist, cls_mask, w_t, "w_t", who);
}

}  // namespace ldw

extern "C" {

int ldw_mi_segment_map(ldw_ctx *c, const int32_t *blocks, int64_t nblocks, int quirk_mode, const int32_t *seg, int32_t S, double sr_dist, int cls_mask, const double *w,
                       double thr, int64_t *n_out, int64_t *nge_out, int64_t *sum_lo_out, int64_t *sum_hi_out, double *max_out, int64_t *npairs_out) {
    const char *who = "ldw_mi_segment_map";
    if (int rc = pair_blocks_check(c, who, blocks, nblocks, quirk_mode, n_out && npairs_out && (sum_lo_out != nullptr) == (sum_hi_out != nullptr),
                                   [&] { return segmap_check(seg, c->L, "seg", S, sr_dist, cls_mask, w, "w", who); }))
        return rc;
    if (int rc = segmap_size(blocks, nblocks, who)) return rc;
    SegRun R;
    R.thr = thr;
    if (int rc = seg_begin(c, R, S, seg, nullptr, w, nullptr, c->L, c->L, nullptr)) return rc;
    PairBlockWalk W;
    if (int rc = seg_walk(c, R, blocks, nblocks, quirk_mode, sr_dist, cls_mask, W)) return rc;
    unsigned long long st[SM_NSTAT];
    if (int rc = map_fetch(c, R, n_out, nge_out, sum_lo_out, sum_hi_out, max_out, st)) return rc;
    *npairs_out = (int64_t)st[5];
    seg_done(c, st, nblocks, W);
    return LDW_OK;
}

int ldw_mi_segment_best(ldw_ctx *c, const int32_t *blocks, int64_t nblocks, int quirk_mode, const int32_t *seg, int32_t S, double sr_dist, int cls_mask, const double *w,
                        const double *max_in, uint64_t *pair_out) {
    const char *who = "ldw_mi_segment_best";
    if (int rc = pair_blocks_check(c, who, blocks, nblocks, quirk_mode, max_in && pair_out, [&] { return segmap_check(seg, c->L, "seg", S, sr_dist, cls_mask, w, "w", who); }))
        return rc;
    if (int rc = segmap_size(blocks, nblocks, who)) return rc;
    SegRun R;
    if (int rc = seg_begin(c, R, S, seg, nullptr, w, nullptr, c->L, c->L, max_in)) return rc;
    PairBlockWalk W;
    if (int rc = seg_walk(c, R, blocks, nblocks, quirk_mode, sr_dist, cls_mask, W)) return rc;
    unsigned long long st[SM_NSTAT];
    if (int rc = best_fetch(c, R, pair_out, st)) return rc;
    seg_done(c, st, nblocks, W);
    return LDW_OK;
}

int ldw_segment_map_report(ldw_ctx *c, int64_t out[5]) {
    LDW_REQUIRE(c && out, LDW_ERR_ARG, "ldw_segment_map_report: null argument");
    for (int k = 0; k < 5; ++k) out[k] = c->segmap_stat[k];
    return LDW_OK;
}

int ldw_debug_segment_map(ldw_ctx *c, const double *mi, int64_t nf, int64_t nt, const int32_t *pos_f, const int32_t *pos_t, double g, int diag, const int32_t *seg_f,
                          const int32_t *seg_t, int32_t S, double sr_dist, int cls_mask, const double *w_f, const double *w_t, double thr, int route, int64_t *n_out,
                          int64_t *nge_out, int64_t *sum_lo_out, int64_t *sum_hi_out, double *max_out, int64_t *npairs_out, int64_t *stats_out) {
    const char *who = "ldw_debug_segment_map";
    if (int rc = check_gpu(c)) return rc;
    if (int rc = seg_debug_check(who, mi, nf, nt, pos_f, pos_t, g, diag, route, seg_f, seg_t, S, sr_dist, cls_mask, w_f, w_t)) return rc;
    LDW_REQUIRE(n_out && npairs_out && (sum_lo_out != nullptr) == (sum_hi_out != nullptr), LDW_ERR_ARG, "%s: null argument", who);
    if (int rc = join_prepare(c)) return rc;
    SegRun R;
    R.thr = thr;
    DevBuf d_mi, d_pf, d_pt;
    if (int rc = seg_begin(c, R, S, seg_f, seg_t, w_f, w_t, nf, nt, nullptr)) return rc;
    if (int rc = upload(c, d_mi, mi, (size_t)(nf * nt))) return rc;
    if (int rc = upload(c, d_pf, pos_f, (size_t)nf)) return rc;
    if (int rc = upload(c, d_pt, pos_t, (size_t)nt)) return rc;
    if (int rc = seg_launch(c, R, d_mi.as<double>(), nf, nt, d_pf.as<int32_t>(), nullptr, nullptr, d_pt.as<int32_t>(), nullptr, nullptr, g, diag, sr_dist, cls_mask, route))
        return rc;
    unsigned long long st[SM_NSTAT];
    if (int rc = map_fetch(c, R, n_out, nge_out, sum_lo_out, sum_hi_out, max_out, st)) return rc;
    LDW_REQUIRE(st[4] == 0, LDW_ERR_ARG, "%s: route 1, but %llu patches hold more than %d row runs or %d column runs", who, st[4], SM_RR, SM_CR);
    *npairs_out = (int64_t)st[5];
    if (stats_out)
        for (int k = 0; k < 4; ++k) stats_out[k] = (int64_t)st[k];
    return LDW_OK;
}

int ldw_debug_segment_best(ldw_ctx *c, const double *mi, int64_t nf, int64_t nt, const int32_t *pos_f, const int32_t *pos_t, double g, int diag, const int32_t *seg_f,
                           const int32_t *seg_t, int32_t S, double sr_dist, int cls_mask, const int32_t *id_f, const int32_t *id_t, const double *w_f, const double *w_t,
                           const double *max_in, int route, uint64_t *pair_out, int64_t *stats_out) {
    const char *who = "ldw_debug_segment_best";
    if (int rc = check_gpu(c)) return rc;
    if (int rc = seg_debug_check(who, mi, nf, nt, pos_f, pos_t, g, diag, route, seg_f, seg_t, S, sr_dist, cls_mask, w_f, w_t)) return rc;
    LDW_REQUIRE(id_f && id_t && max_in && pair_out, LDW_ERR_ARG, "%s: null argument", who);
    for (int64_t i = 0; i < nf; ++i) LDW_REQUIRE(id_f[i] >= 0 && id_f[i] < INT32_MAX, LDW_ERR_ARG, "%s: id_f[%lld] outside 0..2^31 - 2", who, (long long)i);
    for (int64_t i = 0; i < nt; ++i) LDW_REQUIRE(id_t[i] >= 0 && id_t[i] < INT32_MAX, LDW_ERR_ARG, "%s: id_t[%lld] outside 0..2^31 - 2", who, (long long)i);
    if (int rc = join_prepare(c)) return rc;
    SegRun R;
    DevBuf d_mi, d_pf, d_pt, d_if, d_it;
    if (int rc = seg_begin(c, R, S, seg_f, seg_t, w_f, w_t, nf, nt, max_in)) return rc;
    if (int rc = upload(c, d_mi, mi, (size_t)(nf * nt))) return rc;
    if (int rc = upload(c, d_pf, pos_f, (size_t)nf)) return rc;
    if (int rc = upload(c, d_pt, pos_t, (size_t)nt)) return rc;
    if (int rc = upload(c, d_if, id_f, (size_t)nf)) return rc;
    if (int rc = upload(c, d_it, id_t, (size_t)nt)) return rc;
    if (int rc = seg_launch(c, R, d_mi.as<double>(), nf, nt, d_pf.as<int32_t>(), nullptr, d_if.as<int32_t>(), d_pt.as<int32_t>(), nullptr, d_it.as<int32_t>(), g, diag, sr_dist,
                            cls_mask, route))
        return rc;
    unsigned long long st[SM_NSTAT];
    if (int rc = best_fetch(c, R, pair_out, st)) return rc;
    LDW_REQUIRE(st[4] == 0, LDW_ERR_ARG, "%s: route 1, but %llu patches hold more than %d row runs or %d column runs", who, st[4], SM_RR, SM_CR);
    if (stats_out)
        for (int k = 0; k < 4; ++k) stats_out[k] = (int64_t)st[k];
    return LDW_OK;
}

}  // extern "C"
