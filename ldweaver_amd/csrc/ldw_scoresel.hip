// Selection by a corrected score over EVERY SNP pair of a block list (ldweaver_amd.h 22): s = mi - w[A] w[B] (ldw_score.h), w a per-SNP
// vector of the caller's.  Two walks over the blocks and pair set of ldw_mi_profile, each one launch per block behind the block's epilogue, each reading the
// dense block of the plain path (block_mi_dense -> ctx->MIblk, column-major) once:
//   k_score_scan   the histogram of mi_bucket(s) over the pairs inside the class mask and, per SNP, the largest score over its partners (f64_key order);
//   k_score_links  the pairs with s >= thr as a list (from-SNP, to-SNP, mi, s), counted exactly whatever the capacity, and per SNP the smallest partner
//                  whose score has the key of the caller's best_in.
// Every output is an integer add, a maximum of an order-preserving 64-bit key or a 32-bit minimum: no result depends on the order of evaluation, and there
// is no floating-point atomic.
//
// Both kernels keep the patch shape of k_decay_hist and k_snp_summary: a workgroup of four waves takes 64 rows (a_loc, the lanes) x SC_C columns (b_loc; wave w
// takes the SC_WC contiguous columns w * SC_WC ..., eight loads in flight).  The class of a pair is circ_len per pair, never a bound of the patch.
//   scan, histogram   4096 uint32 counters per workgroup in LDS.  Bucket 0 (negatives, +-0, below 2^-20: about half of all pairs) never touches them: its
//                     lanes are counted in a register.  The others go by LDS atomics, the lanes that share the first active lane's counter added as one
//                     (k_decay_hist's route A); then one global add per counter that is not zero.
//   scan, rows        a lane owns its row and keeps its largest key in a register; the four waves combine through LDS, one global maximum per row.
//   scan, columns     k_snp_summary's wave-private transpose, of the keys: a batch of SC_B columns goes to a sub-tile of the wave's own (leading dimension 65:
//                     the read-back is conflict-free), is read back with lane = (column = lane & 15, row quarter = lane >> 4), 16 keys folded in sequence,
//                     the quarters in two cross-lane steps, then one global maximum per column from 16 contiguous lanes.  A pair that takes no part (outside
//                     the pair set or the mask, NaN score) has key 0, which no number's key is.
//   links             a compare per pair; the hits of a column are appended with a ballot and ONE counter add per wave; a key equality against best_in of
//                     the row's SNP (a register) and of the column's SNP (LDS), a 32-bit atomic minimum on a match.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "ldw_internal.h"
#include "ldw_dev.h"
#include "ldw_epi.h"
#include "ldw_score.h"

using namespace ldw;

namespace ldw {

#ifndef LDW_ABLATE_SCORESEL
#define LDW_ABLATE_SCORESEL 0   // measurement builds (make VARIANT=.. EXTRA_DEFS=-DLDW_ABLATE_SCORESEL=n): 1 = the scan counts nothing in LDS; DESIGN.md 33
#endif
constexpr int SC_ROWS = 64;          // rows of a patch: the lanes of a wave
constexpr int SC_C = 256;            // columns of a patch
constexpr int SC_THREADS = 256;
constexpr int SC_WAVES = SC_THREADS / 64;
constexpr int SC_WC = SC_C / SC_WAVES;   // contiguous columns of a wave
constexpr int SC_B = 16;             // columns of a batch: the sub-tile a wave transposes at once
constexpr int SC_U = 8;              // columns a wave has in flight
constexpr int SC_LD = 65;            // keys between two columns of the sub-tile
constexpr int SC_NSTAT = 4;          // [0] patches visited, [1] NaN scores, [2] pairs inside the mask, [3] pairs listed
static_assert(SC_C == SC_THREADS, "every thread fetches the position and the weight of one column of the patch");
static_assert(SC_B == 16 && SC_WC % SC_B == 0 && SC_B % SC_U == 0, "the read-back maps lane -> (column = lane & 15, row quarter = lane >> 4)");
static_assert(SC_WAVES * 64 <= SC_WAVES * SC_B * SC_LD, "the row combine reuses the sub-tiles");

struct ScoreSide {
    const int32_t *pos, *idx;       // the position, the weight, the key and the partner of local index i are those of idx[i] (null: i itself)
    const int32_t *id;              // the global SNP of local index i (the links kernel alone reads it)
    const double *w;
    unsigned long long *key;        // scan: the largest key so far, 0 = none; links: the key of best_in, 0 = NaN (null: no partners wanted)
    int32_t *partner;               // links: the smallest matching partner so far, INT_MAX = none
};

struct ScoreArgs {
    const double *MI;               // [nf * nt] column-major: the pair (a_loc, b_loc) at a_loc + b_loc * nf
    int64_t nf, nt;
    ScoreSide F, T;                 // the from side (rows) and the to side (columns); may share key and partner
    double g, sr_dist;
    int diag;                       // 1: pairs a_loc > b_loc; 0: pairs a_loc != b_loc
    int cls_mask;                   // 1: circ_len <= sr_dist, 2: beyond, 3: both (no distance is computed)
    unsigned long long *hist;       // scan: [NBINS]
    double thr;                     // links
    unsigned long long cap;
    int32_t *la, *lb;
    double *lmi, *ls;
    unsigned long long *stat;       // [SC_NSTAT]
};

__device__ __forceinline__ void sc_max(unsigned long long *p, unsigned long long key) {
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key) atomicMax(p, key);
}
// the pair (a, b) takes part: it is one of the block's pairs and its class is in the mask
__device__ __forceinline__ bool sc_active(const ScoreArgs &A, bool in_patch, int64_t a, int64_t b, int pt, double pf) {
    bool active = in_patch && (A.diag ? a > b : a != b);
    if (A.cls_mask != 3) active = active && ((circ_len((double)pt, pf, A.g) <= A.sr_dist ? 1 : 2) & A.cls_mask) != 0;
    return active;
}

// Three waves per SIMD: three workgroups of 52 736 bytes fit the LDS
__global__ __launch_bounds__(SC_THREADS, 3) void k_score_scan(ScoreArgs A) {
    __shared__ unsigned long long s_tile[SC_WAVES * SC_B * SC_LD];   // the waves' sub-tiles (keys); then the waves' row maxima
    __shared__ uint32_t s_hist[NBINS];
    __shared__ double s_wt[SC_C];   // the weights of the patch's columns
    __shared__ int s_pt[SC_C];      // their positions
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t a0 = (int64_t)blockIdx.x * SC_ROWS, b0 = (int64_t)blockIdx.y * SC_C;
    const int64_t a1 = a0 + SC_ROWS < A.nf ? a0 + SC_ROWS : A.nf, b1 = b0 + SC_C < A.nt ? b0 + SC_C : A.nt;
    if (A.diag && a1 - 1 <= b0) return;   // no pair a_loc > b_loc in the patch
    for (int i = tid; i < NBINS; i += SC_THREADS) s_hist[i] = 0;
    const int64_t a = a0 + lane;
    const bool row_ok = a < a1;
    const int64_t ia = row_ok ? (A.F.idx ? A.F.idx[a] : a) : 0;
    const double pf = row_ok ? (double)A.F.pos[ia] : 0.0, wa = row_ok ? A.F.w[ia] : 0.0;
    if (b0 + tid < b1) {
        const int64_t ib = A.T.idx ? A.T.idx[b0 + tid] : b0 + tid;
        s_pt[tid] = A.T.pos[ib], s_wt[tid] = A.T.w[ib];
    }
    __syncthreads();
    if (tid == 0) atomicAdd(&A.stat[0], 1ull);
    unsigned long long *tile = s_tile + w * (SC_B * SC_LD);
    unsigned long long rkey = 0;          // the largest key of the lane's row over the wave's columns
    uint32_t n_zero = 0, n_nan = 0, n_in = 0;   // of the lane: scores of bucket 0, NaN scores, pairs inside the mask
    const int u_me = lane & 15, qt = lane >> 4;
    const int64_t wb1 = b0 + (int64_t)(w + 1) * SC_WC < b1 ? b0 + (int64_t)(w + 1) * SC_WC : b1;
    for (int64_t bb = b0 + (int64_t)w * SC_WC; bb < wb1; bb += SC_B) {
        if (A.diag && a1 - 1 <= bb) break;   // no pair a_loc > b_loc in this batch or in a later one
#pragma unroll
        for (int h = 0; h < SC_B; h += SC_U) {
            double v[SC_U];
#pragma unroll
            for (int u = 0; u < SC_U; ++u) {
                const int64_t b = bb + h + u;
                v[u] = (b < b1 && row_ok && (A.diag ? a > b : a != b)) ? A.MI[a + b * A.nf] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < SC_U; ++u) {
                const int64_t b = bb + h + u;   // (b - b0 < SC_C: within s_pt and s_wt also past b1, where no lane is active)
                const bool active = sc_active(A, b < b1 && row_ok, a, b, s_pt[b - b0], pf);
                const double s = pair_score(v[u], wa, s_wt[b - b0]);
                const bool valid = active && s == s;
                const unsigned long long key = valid ? f64_key(s) : 0ull;
                const int bk = mi_bucket(s);
                n_in += active, n_nan += active && !valid, n_zero += valid && bk == 0;
                rkey = key > rkey ? key : rkey;
                tile[(h + u) * SC_LD + lane] = key;
#if LDW_ABLATE_SCORESEL != 1
                const bool todo = valid && bk != 0;
                const unsigned long long rem = __ballot(todo);
                if (rem) {   // the lanes that share the first active lane's counter are added as one
                    const int first = __ffsll((long long)rem) - 1;
                    const int k0 = __shfl(bk, first);
                    const unsigned long long same = __ballot(todo && bk == k0);
                    if (lane == first) atomicAdd(&s_hist[k0], (uint32_t)__popcll(same));
                    else if (todo && bk != k0) atomicAdd(&s_hist[bk], 1u);
                }
#endif
            }
        }
        // the sub-tile is the wave's own: its LDS operations complete in order, the fence keeps the compiler from moving them across
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        unsigned long long cm = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const unsigned long long k = tile[u_me * SC_LD + qt * 16 + i];
            cm = k > cm ? k : cm;
        }
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const unsigned long long om = __shfl_xor(cm, o);
            cm = om > cm ? om : cm;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();   // the next batch overwrites the sub-tile
        const int64_t b = bb + lane;
        if (lane < SC_B && b < b1 && cm) sc_max(A.T.key + (A.T.idx ? A.T.idx[b] : b), cm);
    }
    for (int o = 32; o; o >>= 1) n_zero += __shfl_xor(n_zero, o), n_nan += __shfl_xor(n_nan, o), n_in += __shfl_xor(n_in, o);
    if (lane == 0) {
        if (n_zero) atomicAdd(&s_hist[0], n_zero);
        if (n_nan) atomicAdd(&A.stat[1], (unsigned long long)n_nan);
        if (n_in) atomicAdd(&A.stat[2], (unsigned long long)n_in);
    }
    // the four waves' row maxima through LDS
    __syncthreads();
    s_tile[w * 64 + lane] = rkey;
    __syncthreads();
    if (w == 0) {
        unsigned long long t = 0;
#pragma unroll
        for (int v = 0; v < SC_WAVES; ++v) {
            const unsigned long long x = s_tile[v * 64 + lane];
            t = x > t ? x : t;
        }
        if (row_ok && t) sc_max(A.F.key + ia, t);
    }
    for (int i = tid; i < NBINS; i += SC_THREADS) {
        const uint32_t v = s_hist[i];
        if (v) atomicAdd(&A.hist[i], (unsigned long long)v);
    }
}

__global__ __launch_bounds__(SC_THREADS) void k_score_links(ScoreArgs A) {
    __shared__ unsigned long long s_bk[SC_C];   // the keys of best_in of the patch's columns
    __shared__ double s_wt[SC_C];
    __shared__ int s_pt[SC_C], s_id[SC_C];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t a0 = (int64_t)blockIdx.x * SC_ROWS, b0 = (int64_t)blockIdx.y * SC_C;
    const int64_t a1 = a0 + SC_ROWS < A.nf ? a0 + SC_ROWS : A.nf, b1 = b0 + SC_C < A.nt ? b0 + SC_C : A.nt;
    if (A.diag && a1 - 1 <= b0) return;   // no pair a_loc > b_loc in the patch
    const bool partners = A.F.key != nullptr;
    const int64_t a = a0 + lane;
    const bool row_ok = a < a1;
    const int64_t ia = row_ok ? (A.F.idx ? A.F.idx[a] : a) : 0;
    const double pf = row_ok ? (double)A.F.pos[ia] : 0.0, wa = row_ok ? A.F.w[ia] : 0.0;
    const int id_a = row_ok ? A.F.id[a] : 0;
    const unsigned long long bk_a = partners && row_ok ? A.F.key[ia] : 0ull;
    if (b0 + tid < b1) {
        const int64_t ib = A.T.idx ? A.T.idx[b0 + tid] : b0 + tid;
        s_pt[tid] = A.T.pos[ib], s_wt[tid] = A.T.w[ib], s_id[tid] = A.T.id[b0 + tid];
        s_bk[tid] = partners ? A.T.key[ib] : 0ull;
    }
    __syncthreads();
    if (tid == 0) atomicAdd(&A.stat[0], 1ull);
    uint32_t n_nan = 0;
    const int64_t wb1 = b0 + (int64_t)(w + 1) * SC_WC < b1 ? b0 + (int64_t)(w + 1) * SC_WC : b1;
    for (int64_t bb = b0 + (int64_t)w * SC_WC; bb < wb1; bb += SC_U) {
        if (A.diag && a1 - 1 <= bb) break;   // no pair a_loc > b_loc in these columns or in later ones
        double v[SC_U];
#pragma unroll
        for (int u = 0; u < SC_U; ++u) {
            const int64_t b = bb + u;
            v[u] = (b < b1 && row_ok && (A.diag ? a > b : a != b)) ? A.MI[a + b * A.nf] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < SC_U; ++u) {
            const int64_t b = bb + u;   // (b - b0 < SC_C: within the LDS arrays also past b1, where no lane is active)
            const bool active = sc_active(A, b < b1 && row_ok, a, b, s_pt[b - b0], pf);
            const double s = pair_score(v[u], wa, s_wt[b - b0]);
            const bool valid = active && s == s;
            n_nan += active && !valid;
            const bool hit = active && s >= A.thr;   // (an fp64 comparison: false for a NaN score and for a NaN threshold)
            const unsigned long long bal = __ballot(hit);
            if (bal) {   // one counter add per wave; the hits take consecutive places
                const int first = __ffsll((long long)bal) - 1;
                unsigned long long base = 0;
                if (lane == first) base = atomicAdd(&A.stat[3], (unsigned long long)__popcll(bal));
                base = __shfl(base, first);
                const unsigned long long at = base + (unsigned long long)__popcll(bal & ((1ull << lane) - 1ull));
                if (hit && at < A.cap) A.la[at] = id_a, A.lb[at] = s_id[b - b0], A.lmi[at] = v[u], A.ls[at] = s;
            }
            if (partners && valid) {
                const unsigned long long key = f64_key(s);
                if (key == bk_a) atomicMin(&A.F.partner[ia], s_id[b - b0]);
                if (key == s_bk[b - b0]) atomicMin(&A.T.partner[A.T.idx ? (int64_t)s_id[b - b0] : b], id_a);
            }
        }
    }
    for (int o = 32; o; o >>= 1) n_nan += __shfl_xor(n_nan, o);
    if (lane == 0 && n_nan) atomicAdd(&A.stat[1], (unsigned long long)n_nan);
}

// One walk: the per-SNP vectors staged once, the device-side results and counters
struct ScoreRun {
    DevBuf w_f, w_t, key_f, key_t, part_f, part_t, hist, stat, la, lb, lmi, ls;
    int64_t lenF = 0, lenT = 0;
    bool shared = false;   // both sides use the from side's vectors (the SNPs of an alignment); else rows and columns apart (the debug entries)
    bool links = false, partners = false;
    double thr = 0;
    int64_t cap = 0;
};

static int score_check(double sr_dist, int cls_mask, const double *w, int64_t n, const char *wname, const char *who) {
    LDW_REQUIRE(!std::isnan(sr_dist) && sr_dist >= 0, LDW_ERR_ARG, "%s: sr_dist must be a non-negative number (+inf allowed)", who);
    LDW_REQUIRE(cls_mask >= 1 && cls_mask <= 3, LDW_ERR_ARG, "%s: cls_mask %d outside 1..3", who, cls_mask);
    LDW_REQUIRE(w, LDW_ERR_ARG, "%s: null %s", who, wname);
    for (int64_t i = 0; i < n; ++i) LDW_REQUIRE(std::isfinite(w[i]), LDW_ERR_ARG, "%s: %s[%lld] is not finite", who, wname, (long long)i);
    return LDW_OK;
}

static int links_check(int64_t cap, const void *a, const void *b, const void *mi, const void *s, const void *count, const void *best, const void *partner, const char *who) {
    LDW_REQUIRE(count, LDW_ERR_ARG, "%s: null count_out", who);
    LDW_REQUIRE(cap >= 0 && (cap == 0 || (a && b && mi && s)), LDW_ERR_ARG, "%s: cap %lld needs the four lists", who, (long long)cap);
    LDW_REQUIRE(!partner || best, LDW_ERR_ARG, "%s: partner_out needs best_in", who);
    return LDW_OK;
}

static std::vector<unsigned long long> best_keys(const double *best, int64_t n) {   // 0 for NaN: no score has that key
    std::vector<unsigned long long> k((size_t)n);
    for (int64_t i = 0; i < n; ++i) k[(size_t)i] = std::isnan(best[i]) ? 0ull : (unsigned long long)f64_key(best[i]);
    return k;
}

// the per-SNP vectors of one side to the device; best: null for a scan (the keys start at 0) or for links without partners
static int score_side(ldw_ctx *c, const ScoreRun &R, DevBuf &w_buf, DevBuf &key_buf, DevBuf &part_buf, const double *w, const double *best, int64_t len) {
    if (int rc = upload(c, w_buf, w, (size_t)len)) return rc;
    if (!R.links) {
        if (int rc = key_buf.reserve((size_t)len * 8)) return rc;
        LDW_HIP(hipMemsetAsync(key_buf.p, 0, (size_t)len * 8, c->stream));
    } else if (R.partners) {
        const std::vector<unsigned long long> k = best_keys(best, len);
        if (int rc = upload(c, key_buf, k.data(), (size_t)len)) return rc;
        LDW_HIP(hipStreamSynchronize(c->stream));   // (k goes with this frame)
        if (int rc = part_buf.reserve((size_t)len * 4)) return rc;
        LDW_HIP(hipMemsetD32Async((hipDeviceptr_t)part_buf.p, INT_MAX, (size_t)len, c->stream));
    }
    return LDW_OK;
}

static int score_begin(ldw_ctx *c, ScoreRun &R, const double *w_f, const double *w_t, const double *best_f, const double *best_t, int64_t lenF, int64_t lenT, bool shared) {
    R.lenF = lenF, R.lenT = shared ? lenF : lenT, R.shared = shared;
    if (int rc = score_side(c, R, R.w_f, R.key_f, R.part_f, w_f, best_f, R.lenF)) return rc;
    if (!shared)
        if (int rc = score_side(c, R, R.w_t, R.key_t, R.part_t, w_t, best_t, R.lenT)) return rc;
    if (int rc = R.stat.reserve(SC_NSTAT * 8)) return rc;
    LDW_HIP(hipMemsetAsync(R.stat.p, 0, SC_NSTAT * 8, c->stream));
    if (!R.links) {
        if (int rc = R.hist.reserve((size_t)NBINS * 8)) return rc;
        LDW_HIP(hipMemsetAsync(R.hist.p, 0, (size_t)NBINS * 8, c->stream));
    } else {
        const size_t n = (size_t)std::max<int64_t>(R.cap, 1);
        if (int rc = R.la.reserve(n * 4)) return rc;
        if (int rc = R.lb.reserve(n * 4)) return rc;
        if (int rc = R.lmi.reserve(n * 8)) return rc;
        if (int rc = R.ls.reserve(n * 8)) return rc;
    }
    return LDW_OK;
}

static int score_launch(ldw_ctx *c, const ScoreRun &R, const double *MI, int64_t nf, int64_t nt, const int32_t *pos_f, const int32_t *idx_f, const int32_t *id_f,
                        const int32_t *pos_t, const int32_t *idx_t, const int32_t *id_t, double g, int diag, double sr_dist, int cls_mask) {
    ScoreArgs A;
    const bool keys = !R.links || R.partners;
    A.MI = MI, A.nf = nf, A.nt = nt;
    A.F.pos = pos_f, A.F.idx = idx_f, A.F.id = id_f, A.F.w = R.w_f.as<double>();
    A.F.key = keys ? R.key_f.as<unsigned long long>() : nullptr, A.F.partner = R.part_f.as<int32_t>();
    A.T.pos = pos_t, A.T.idx = idx_t, A.T.id = id_t, A.T.w = (R.shared ? R.w_f : R.w_t).as<double>();
    A.T.key = keys ? (R.shared ? R.key_f : R.key_t).as<unsigned long long>() : nullptr, A.T.partner = (R.shared ? R.part_f : R.part_t).as<int32_t>();
    A.g = g, A.sr_dist = sr_dist, A.diag = diag, A.cls_mask = cls_mask;
    A.hist = R.hist.as<unsigned long long>();
    A.thr = R.thr, A.cap = (unsigned long long)R.cap;
    A.la = R.la.as<int32_t>(), A.lb = R.lb.as<int32_t>(), A.lmi = R.lmi.as<double>(), A.ls = R.ls.as<double>();
    A.stat = R.stat.as<unsigned long long>();
    const dim3 grid((unsigned)((nf + SC_ROWS - 1) / SC_ROWS), (unsigned)((nt + SC_C - 1) / SC_C));
    if (R.links) hipLaunchKernelGGL(k_score_links, grid, dim3(SC_THREADS), 0, c->stream, A);
    else hipLaunchKernelGGL(k_score_scan, grid, dim3(SC_THREADS), 0, c->stream, A);
    LDW_HIP(hipGetLastError());
    return LDW_OK;
}

// the largest scores of one side from their keys (NaN where there is none); the stream is synchronised
static int scan_best(ldw_ctx *c, const DevBuf &key, int64_t len, double *best_out) {
    std::vector<unsigned long long> k((size_t)len);
    LDW_HIP(hipMemcpyAsync(k.data(), key.p, (size_t)len * 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < len; ++i) best_out[i] = k[(size_t)i] ? key_f64(k[(size_t)i]) : std::nan("");
    return LDW_OK;
}

// the partners of one side (-1 where there is none); the stream is synchronised
static int links_partner(ldw_ctx *c, const DevBuf &part, int64_t len, int32_t *partner_out) {
    LDW_HIP(hipMemcpyAsync(partner_out, part.p, (size_t)len * 4, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < len; ++i)
        if (partner_out[i] == INT_MAX) partner_out[i] = -1;
    return LDW_OK;
}

// the counters, then the list when it fits: LDW_ERR_SIZE (count written, lists undefined) when it does not
static int links_fetch(ldw_ctx *c, const ScoreRun &R, unsigned long long st[SC_NSTAT], int32_t *a_out, int32_t *b_out, double *mi_out, double *score_out, int64_t *count_out,
                       const char *who) {
    LDW_HIP(hipMemcpyAsync(st, R.stat.p, SC_NSTAT * 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    const int64_t n = (int64_t)st[3];
    *count_out = n;
    if (R.cap == 0 && !a_out) return LDW_OK;   // a pure count
    LDW_REQUIRE(n <= R.cap, LDW_ERR_SIZE, "%s: %lld pairs at or above the threshold, cap %lld", who, (long long)n, (long long)R.cap);
    if (n) {
        LDW_HIP(hipMemcpyAsync(a_out, R.la.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipMemcpyAsync(b_out, R.lb.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipMemcpyAsync(mi_out, R.lmi.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipMemcpyAsync(score_out, R.ls.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipStreamSynchronize(c->stream));
    }
    return LDW_OK;
}

static void score_done(ldw_ctx *c, const unsigned long long st[SC_NSTAT], int64_t nblocks, const PairBlockWalk &W) {
    c->scoresel_stat[0] = (int64_t)st[0], c->scoresel_stat[1] = (int64_t)st[1], c->scoresel_stat[2] = nblocks;
    c->last_ms[0] = W.ms_mi, c->last_ms[1] = W.ms_consumer, c->last_ms[2] = 0, c->last_ms[3] = W.ms_mi + W.ms_consumer;
}

static int debug_check(const char *who, const void *mi, int64_t nf, int64_t nt, const void *pos_f, const void *pos_t, double g, int diag) {
    LDW_REQUIRE(mi && pos_f && pos_t, LDW_ERR_ARG, "%s: null argument", who);
    LDW_REQUIRE(nf >= 1 && nt >= 1 && nf <= 1000000 && nt <= 1000000, LDW_ERR_ARG, "%s: nf, nt outside 1..1 000 000", who);
    LDW_REQUIRE(diag == 0 || (diag == 1 && nf == nt), LDW_ERR_ARG, "%s: diag is 0 or 1, and a diagonal block is square", who);
    LDW_REQUIRE(std::isfinite(g) && g > 0, LDW_ERR_ARG, "%s: g must be positive", who);
    return LDW_OK;
}

}  // namespace ldw

extern "C" {

int ldw_mi_score_scan(ldw_ctx *c, const int32_t *blocks, int64_t nblocks, int quirk_mode, double sr_dist, int cls_mask, const double *w, uint64_t *hist_out,
                      double *best_out, int64_t *npairs_out) {
    const char *who = "ldw_mi_score_scan";
    if (int rc = pair_blocks_check(c, who, blocks, nblocks, quirk_mode, hist_out && best_out && npairs_out, [&] { return score_check(sr_dist, cls_mask, w, c->L, "w", who); }))
        return rc;
    ScoreRun R;
    if (int rc = score_begin(c, R, w, nullptr, nullptr, nullptr, c->L, c->L, true)) return rc;
    PairBlockWalk W;
    if (int rc = pair_blocks_walk(c, blocks, nblocks, quirk_mode, W, [&](int64_t nf, int64_t nt, bool diag) {
            return score_launch(c, R, c->MIblk.as<double>(), nf, nt, c->meta.POS.as<int32_t>(), c->idx_f.as<int32_t>(), c->idx_f.as<int32_t>(), c->meta.POS.as<int32_t>(),
                                c->idx_t.as<int32_t>(), c->idx_t.as<int32_t>(), c->meta.g, diag ? 1 : 0, sr_dist, cls_mask);
        }))
        return rc;
    unsigned long long st[SC_NSTAT];
    LDW_HIP(hipMemcpyAsync(hist_out, R.hist.p, (size_t)NBINS * 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemcpyAsync(st, R.stat.p, sizeof st, hipMemcpyDeviceToHost, c->stream));
    if (int rc = scan_best(c, R.key_f, c->L, best_out)) return rc;
    *npairs_out = (int64_t)st[2];
    score_done(c, st, nblocks, W);
    return LDW_OK;
}

int ldw_mi_score_links(ldw_ctx *c, const int32_t *blocks, int64_t nblocks, int quirk_mode, double sr_dist, int cls_mask, const double *w, double thr, const double *best_in,
                       int64_t cap, int32_t *a_out, int32_t *b_out, double *mi_out, double *score_out, int64_t *count_out, int32_t *partner_out) {
    const char *who = "ldw_mi_score_links";
    if (int rc = pair_blocks_check(c, who, blocks, nblocks, quirk_mode, true, [&] {
            if (int rc2 = score_check(sr_dist, cls_mask, w, c->L, "w", who)) return rc2;
            return links_check(cap, a_out, b_out, mi_out, score_out, count_out, best_in, partner_out, who);
        }))
        return rc;
    ScoreRun R;
    R.links = true, R.partners = partner_out != nullptr, R.thr = thr, R.cap = cap;
    if (int rc = score_begin(c, R, w, nullptr, best_in, nullptr, c->L, c->L, true)) return rc;
    PairBlockWalk W;
    if (int rc = pair_blocks_walk(c, blocks, nblocks, quirk_mode, W, [&](int64_t nf, int64_t nt, bool diag) {
            return score_launch(c, R, c->MIblk.as<double>(), nf, nt, c->meta.POS.as<int32_t>(), c->idx_f.as<int32_t>(), c->idx_f.as<int32_t>(), c->meta.POS.as<int32_t>(),
                                c->idx_t.as<int32_t>(), c->idx_t.as<int32_t>(), c->meta.g, diag ? 1 : 0, sr_dist, cls_mask);
        }))
        return rc;
    if (partner_out)
        if (int rc = links_partner(c, R.part_f, c->L, partner_out)) return rc;
    unsigned long long st[SC_NSTAT];
    const int rc = links_fetch(c, R, st, a_out, b_out, mi_out, score_out, count_out, who);
    if (rc == LDW_OK || rc == LDW_ERR_SIZE) score_done(c, st, nblocks, W);
    return rc;
}

int ldw_score_select_report(ldw_ctx *c, int64_t out[3]) {
    LDW_REQUIRE(c && out, LDW_ERR_ARG, "ldw_score_select_report: null argument");
    for (int k = 0; k < 3; ++k) out[k] = c->scoresel_stat[k];
    return LDW_OK;
}

int ldw_debug_score_scan(ldw_ctx *c, const double *mi, int64_t nf, int64_t nt, const int32_t *pos_f, const int32_t *pos_t, double g, int diag, double sr_dist, int cls_mask,
                         const double *w_f, const double *w_t, uint64_t *hist_out, double *best_f, double *best_t, int64_t *npairs_out, int64_t *stats_out) {
    const char *who = "ldw_debug_score_scan";
    if (int rc = check_gpu(c)) return rc;
    if (int rc = debug_check(who, mi, nf, nt, pos_f, pos_t, g, diag)) return rc;
    LDW_REQUIRE(hist_out && best_f && best_t && npairs_out, LDW_ERR_ARG, "%s: null argument", who);
    if (int rc = score_check(sr_dist, cls_mask, w_f, nf, "w_f", who)) return rc;
    if (int rc = score_check(sr_dist, cls_mask, w_t, nt, "w_t", who)) return rc;
    if (int rc = join_prepare(c)) return rc;
    ScoreRun R;
    DevBuf d_mi, d_pf, d_pt;
    if (int rc = score_begin(c, R, w_f, w_t, nullptr, nullptr, nf, nt, false)) return rc;
    if (int rc = upload(c, d_mi, mi, (size_t)(nf * nt))) return rc;
    if (int rc = upload(c, d_pf, pos_f, (size_t)nf)) return rc;
    if (int rc = upload(c, d_pt, pos_t, (size_t)nt)) return rc;
    if (int rc = score_launch(c, R, d_mi.as<double>(), nf, nt, d_pf.as<int32_t>(), nullptr, nullptr, d_pt.as<int32_t>(), nullptr, nullptr, g, diag, sr_dist, cls_mask)) return rc;
    unsigned long long st[SC_NSTAT];
    LDW_HIP(hipMemcpyAsync(hist_out, R.hist.p, (size_t)NBINS * 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemcpyAsync(st, R.stat.p, sizeof st, hipMemcpyDeviceToHost, c->stream));
    if (int rc = scan_best(c, R.key_f, nf, best_f)) return rc;
    if (int rc = scan_best(c, R.key_t, nt, best_t)) return rc;
    *npairs_out = (int64_t)st[2];
    if (stats_out) stats_out[0] = (int64_t)st[0], stats_out[1] = (int64_t)st[1];
    return LDW_OK;
}

int ldw_debug_score_links(ldw_ctx *c, const double *mi, int64_t nf, int64_t nt, const int32_t *pos_f, const int32_t *pos_t, double g, int diag, double sr_dist, int cls_mask,
                          const int32_t *id_f, const int32_t *id_t, const double *w_f, const double *w_t, double thr, const double *best_f, const double *best_t, int64_t cap,
                          int32_t *a_out, int32_t *b_out, double *mi_out, double *score_out, int64_t *count_out, int32_t *partner_f, int32_t *partner_t, int64_t *stats_out) {
    const char *who = "ldw_debug_score_links";
    if (int rc = check_gpu(c)) return rc;
    if (int rc = debug_check(who, mi, nf, nt, pos_f, pos_t, g, diag)) return rc;
    LDW_REQUIRE(id_f && id_t, LDW_ERR_ARG, "%s: null argument", who);
    for (int64_t i = 0; i < nf; ++i) LDW_REQUIRE(id_f[i] >= 0 && id_f[i] < INT_MAX, LDW_ERR_ARG, "%s: id_f[%lld] outside 0..2^31 - 2", who, (long long)i);
    for (int64_t i = 0; i < nt; ++i) LDW_REQUIRE(id_t[i] >= 0 && id_t[i] < INT_MAX, LDW_ERR_ARG, "%s: id_t[%lld] outside 0..2^31 - 2", who, (long long)i);
    if (int rc = score_check(sr_dist, cls_mask, w_f, nf, "w_f", who)) return rc;
    if (int rc = score_check(sr_dist, cls_mask, w_t, nt, "w_t", who)) return rc;
    LDW_REQUIRE((partner_f != nullptr) == (partner_t != nullptr) && (best_f != nullptr) == (best_t != nullptr), LDW_ERR_ARG, "%s: the two sides' partners and bests go together", who);
    if (int rc = links_check(cap, a_out, b_out, mi_out, score_out, count_out, best_f, partner_f, who)) return rc;
    if (int rc = join_prepare(c)) return rc;
    ScoreRun R;
    R.links = true, R.partners = partner_f != nullptr, R.thr = thr, R.cap = cap;
    DevBuf d_mi, d_pf, d_pt, d_if, d_it;
    if (int rc = score_begin(c, R, w_f, w_t, best_f, best_t, nf, nt, false)) return rc;
    if (int rc = upload(c, d_mi, mi, (size_t)(nf * nt))) return rc;
    if (int rc = upload(c, d_pf, pos_f, (size_t)nf)) return rc;
    if (int rc = upload(c, d_pt, pos_t, (size_t)nt)) return rc;
    if (int rc = upload(c, d_if, id_f, (size_t)nf)) return rc;
    if (int rc = upload(c, d_it, id_t, (size_t)nt)) return rc;
    if (int rc = score_launch(c, R, d_mi.as<double>(), nf, nt, d_pf.as<int32_t>(), nullptr, d_if.as<int32_t>(), d_pt.as<int32_t>(), nullptr, d_it.as<int32_t>(), g, diag, sr_dist,
                              cls_mask))
        return rc;
    if (partner_f) {
        if (int rc = links_partner(c, R.part_f, nf, partner_f)) return rc;
        if (int rc = links_partner(c, R.part_t, nt, partner_t)) return rc;
    }
    unsigned long long st[SC_NSTAT];
    const int rc = links_fetch(c, R, st, a_out, b_out, mi_out, score_out, count_out, who);
    if ((rc == LDW_OK || rc == LDW_ERR_SIZE) && stats_out) stats_out[0] = (int64_t)st[0], stats_out[1] = (int64_t)st[1];
    return rc;
}

}  // extern "C"
