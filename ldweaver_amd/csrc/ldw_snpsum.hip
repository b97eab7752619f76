// Per-SNP MI summary (ldweaver_amd.h 21): for every SNP and each of the two distance classes (0: circ_len <= sr_dist, 1: beyond) the number of
// partners, the sum of their MI in 40-bit fixed point (ldw_snpsum.h), the largest MI and the number of partners at or above a threshold, over EVERY SNP pair
// of a block list.  The values are the dense block of the plain path (block_mi_dense -> ctx->MIblk, column-major), as in ldw_decay.hip; every pair adds to
// both of its SNPs.  Every output is an integer add or a maximum of an order-preserving 64-bit key: no result depends on the order of the adds.
//
// k_snp_summary: a workgroup of four waves takes a patch of 64 rows (a_loc, the lanes) x SS_C columns (b_loc; wave w takes the SS_WC contiguous columns
// w * SS_WC ..., in batches of SS_B).
//   row side     a lane owns its row and accumulates its columns in registers; the four waves combine through LDS, then one global add or maximum per
//                (row, class, quantity) that is not zero.
//   column side  the 64 lanes of a wave hold the 64 values of one column.  The wave writes the raw values of a batch as an SS_B x 64 sub-tile of its own
//                in LDS (leading dimension 65 doubles: the read-back is conflict-free), keeps per column the ballot of the lanes that hold a pair of each
//                class, and reads the tile back with lane = (column = lane & 15, row quarter = lane >> 4): 16 rows summed in sequence, the four quarters
//                folded in two cross-lane steps, then one global add or maximum per (column, class, quantity) that is not zero from 16 contiguous lanes.
// From the extreme positions of its rows and columns a patch bounds its circular distances (the interval argument of k_decay_hist) and takes one of two routes:
//   (1) the bound puts the whole patch in one class: one set of accumulators;
//   (2) else: both classes are carried.
// Both compute circ_len per pair and never trust the bound: on route 1 a pair whose own class is not the patch's (rounding, a fractional g) is added
// straight to the global accumulators and counted (stat[2]).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ldw_internal.h"
#include "ldw_dev.h"
#include "ldw_snpsum.h"

using namespace ldw;

namespace ldw {

#ifndef LDW_ABLATE_SNPSUM
#define LDW_ABLATE_SNPSUM 0   // measurement builds (make VARIANT=.. EXTRA_DEFS=-DLDW_ABLATE_SNPSUM=n): 1 = no column side, 2 = no global add or maximum; DESIGN.md 32
#endif
constexpr int SS_ROWS = 64;          // rows of a patch: the lanes of a wave
constexpr int SS_C = 256;            // columns of a patch
constexpr int SS_THREADS = 256;
constexpr int SS_WAVES = SS_THREADS / 64;
constexpr int SS_WC = SS_C / SS_WAVES;   // contiguous columns of a wave
constexpr int SS_B = 16;             // columns of a batch: the sub-tile a wave transposes at once
constexpr int SS_U = 8;              // columns a wave has in flight
constexpr int SS_LD = 65;            // doubles between two columns of the sub-tile
constexpr int SS_NQ = 4;             // quantities: partners, sum of q, key of the maximum, partners at or above the threshold
static_assert(SS_C == SS_THREADS, "every thread fetches the position of one column of the patch");
static_assert(SS_B == 16 && SS_WC % SS_B == 0 && SS_B % SS_U == 0, "the read-back maps lane -> (column = lane & 15, row quarter = lane >> 4)");
static_assert(SS_WAVES * 2 * SS_NQ * 64 <= SS_WAVES * SS_B * SS_LD, "the row combine reuses the sub-tiles");

struct SnpSumSide {
    unsigned long long *acc;        // [SS_NQ][2][len]: quantity, class, SNP
    int64_t len;
    const int32_t *pos, *idx;       // the position and the accumulator of local index i are those of idx[i] (null: i itself)
    __device__ __forceinline__ unsigned long long *at(int q, int c, int64_t i) const { return acc + ((size_t)(q * 2 + c) * (size_t)len + (size_t)i); }
};

struct SnpSumArgs {
    const double *MI;               // [nf * nt] column-major: the pair (a_loc, b_loc) at a_loc + b_loc * nf
    int64_t nf, nt;
    SnpSumSide F, T;                // the from side (rows) and the to side (columns); may share acc
    double g, sr_dist, thr0, thr1;
    int diag;                       // 1: pairs a_loc > b_loc; 0: pairs a_loc != b_loc
    int route;                      // 0: the patch chooses; 1: single class or refuse; 2: general
    unsigned long long *stat;       // [0] patches visited, [1] general-route patches, [2] pairs off their patch's class, [3] values q refused, [4] patches route 1 refused,
};                                  // [5], [6] pairs of class 0, 1

__device__ __forceinline__ void ss_add(unsigned long long *p, unsigned long long v) {
#if LDW_ABLATE_SNPSUM != 2
    atomicAdd(p, v);
#endif
}
__device__ __forceinline__ void ss_max(unsigned long long *p, unsigned long long key) {
#if LDW_ABLATE_SNPSUM != 2
    if (__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key) atomicMax(p, key);
#endif
}
// one pair's contribution straight to the accumulators of SNP i of a side
__device__ __forceinline__ void ss_direct(const SnpSumSide &S, int c, int64_t i, long long q, unsigned long long key, bool ge) {
    ss_add(S.at(0, c, i), 1ull);
    if (q) ss_add(S.at(1, c, i), (unsigned long long)q);
    ss_max(S.at(2, c, i), key);
    if (ge) ss_add(S.at(3, c, i), 1ull);
}

// The columns of wave w of a patch.  NC = 1: every pair is of class P (route 1); NC = 2: slot = class (route 2).  tile: the wave's own sub-tile.  Leaves the
// lane's row sums per class in rn, rs, rm, rg and the number of values q refused in refused.
template <int NC>
__device__ __forceinline__ void ss_columns(const SnpSumArgs &A, const int P, unsigned long long *tile, const int *s_pt, const int64_t a, const int64_t a1, const bool row_ok,
                                           const double pf, const int64_t b0, const int64_t b1, const int lane, const int w, uint32_t rn[2], long long rs[2],
                                           unsigned long long rm[2], uint32_t rg[2], uint32_t &refused) {
    uint32_t n_[NC], g_[NC];
    long long s_[NC];
    unsigned long long m_[NC];
#pragma unroll
    for (int s = 0; s < NC; ++s) n_[s] = g_[s] = 0, s_[s] = 0, m_[s] = 0;
    const double thr_p = P ? A.thr1 : A.thr0;   // (NC = 1: the threshold of the patch's class)
    const int u_me = lane & 15, qt = lane >> 4;
    const int64_t wb1 = b0 + (int64_t)(w + 1) * SS_WC < b1 ? b0 + (int64_t)(w + 1) * SS_WC : b1;
    for (int64_t bb = b0 + (int64_t)w * SS_WC; bb < wb1; bb += SS_B) {
        if (A.diag && a1 - 1 <= bb) break;   // no pair a_loc > b_loc in this batch or in a later one
        unsigned long long mk[NC];           // of column u_me of the batch: the lanes (rows) that hold a pair of the slot
#pragma unroll
        for (int s = 0; s < NC; ++s) mk[s] = 0;
#pragma unroll
        for (int h = 0; h < SS_B; h += SS_U) {
            // SS_U columns are loaded before the first is consumed (k_decay_hist: one 512-byte load in flight per wave leaves the kernel waiting for memory)
            double v[SS_U];
#pragma unroll
            for (int u = 0; u < SS_U; ++u) {
                const int64_t b = bb + h + u;
                v[u] = (b < b1 && row_ok && (A.diag ? a > b : a != b)) ? A.MI[a + b * A.nf] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < SS_U; ++u) {
                const int64_t b = bb + h + u;   // (b - b0 < SS_C: within s_pt also past b1, where no lane is active)
                bool active = b < b1 && row_ok && (A.diag ? a > b : a != b);
                const double mi = v[u];
                const int cls = circ_len((double)s_pt[b - b0], pf, A.g) <= A.sr_dist ? 0 : 1;
                bool ref;
                const long long q = snpsum_q(mi, &ref);
                const unsigned long long key = f64_key(mi);
                const bool ge = mi >= (cls ? A.thr1 : A.thr0);
                refused += active && ref;
                if (NC == 1 && active && cls != P) {   // (never in exact arithmetic; no known input reaches it, so no test does: DESIGN.md 32)
                    ss_direct(A.F, cls, A.F.idx ? A.F.idx[a] : a, q, key, ge);
                    ss_direct(A.T, cls, A.T.idx ? A.T.idx[b] : b, q, key, ge);
                    atomicAdd(&A.stat[2], 1ull);
                    atomicAdd(&A.stat[5 + cls], 1ull);
                    active = false;
                }
#pragma unroll
                for (int s = 0; s < NC; ++s) {
                    const bool hit = active && (NC == 1 || cls == s);
                    n_[s] += hit, g_[s] += hit && ge;
                    s_[s] += hit ? q : 0;
                    m_[s] = hit && key > m_[s] ? key : m_[s];
                    const unsigned long long bal = __ballot(hit);
                    if (u_me == h + u) mk[s] = bal;
                }
                tile[(h + u) * SS_LD + lane] = (unsigned long long)__double_as_longlong(mi);
            }
        }
#if LDW_ABLATE_SNPSUM != 1
        // the sub-tile is the wave's own: its LDS operations complete in order, the fence keeps the compiler from moving them across
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        uint32_t cg[NC];
        long long cs[NC];
        unsigned long long cm[NC], mq[NC];
#pragma unroll
        for (int s = 0; s < NC; ++s) cg[s] = 0, cs[s] = 0, cm[s] = 0, mq[s] = mk[s] >> (qt * 16);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const double x = __longlong_as_double((long long)tile[u_me * SS_LD + qt * 16 + i]);
            bool ref;
            const long long q = snpsum_q(x, &ref);
            const unsigned long long key = f64_key(x);
#pragma unroll
            for (int s = 0; s < NC; ++s) {
                const bool hit = (mq[s] >> i) & 1;
                cs[s] += hit ? q : 0;
                cm[s] = hit && key > cm[s] ? key : cm[s];
                cg[s] += hit && x >= (NC == 2 ? (s ? A.thr1 : A.thr0) : thr_p);
            }
        }
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
#pragma unroll
            for (int s = 0; s < NC; ++s) {
                cs[s] += __shfl_xor(cs[s], o);
                const unsigned long long om = __shfl_xor(cm[s], o);
                cm[s] = om > cm[s] ? om : cm[s];
                cg[s] += __shfl_xor(cg[s], o);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();   // the next batch overwrites the sub-tile
        const int64_t b = bb + lane;
        if (lane < SS_B && b < b1) {
            const int64_t ib = A.T.idx ? A.T.idx[b] : b;
#pragma unroll
            for (int s = 0; s < NC; ++s) {
                const int c = NC == 2 ? s : P;
                const int cn = __popcll(mk[s]);
                if (cn) {
                    ss_add(A.T.at(0, c, ib), (unsigned long long)cn);
                    if (cs[s]) ss_add(A.T.at(1, c, ib), (unsigned long long)cs[s]);
                    ss_max(A.T.at(2, c, ib), cm[s]);
                    if (cg[s]) ss_add(A.T.at(3, c, ib), (unsigned long long)cg[s]);
                }
            }
        }
#endif
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if constexpr (NC == 2) {
            rn[c] = n_[c], rs[c] = s_[c], rm[c] = m_[c], rg[c] = g_[c];
        } else {
            const bool mine = c == P;
            rn[c] = mine ? n_[0] : 0, rs[c] = mine ? s_[0] : 0, rm[c] = mine ? m_[0] : 0, rg[c] = mine ? g_[0] : 0;
        }
    }
}

// Three waves per SIMD: unbounded the compiler takes 182 registers (two waves per SIMD, no scratch) and the kernel runs 14 % longer than under this bound
// (168 registers, 48 bytes of scratch per lane); three workgroups of 34 320 bytes fit the LDS.
__global__ __launch_bounds__(SS_THREADS, 3) void k_snp_summary(SnpSumArgs A) {
    __shared__ unsigned long long s_tile[SS_WAVES * SS_B * SS_LD];   // the waves' sub-tiles (raw doubles); then the waves' row sums
    __shared__ int s_ext[4];      // min / max position of the rows, of the columns
    __shared__ int s_pt[SS_C];    // the positions of the patch's columns
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t a0 = (int64_t)blockIdx.x * SS_ROWS, b0 = (int64_t)blockIdx.y * SS_C;
    const int64_t a1 = a0 + SS_ROWS < A.nf ? a0 + SS_ROWS : A.nf, b1 = b0 + SS_C < A.nt ? b0 + SS_C : A.nt;
    if (A.diag && a1 - 1 <= b0) return;   // no pair a_loc > b_loc in the patch
    if (tid == 0) s_ext[0] = s_ext[2] = 0x7FFFFFFF, s_ext[1] = s_ext[3] = (int)0x80000000;
    __syncthreads();
    const int64_t a = a0 + lane;
    const bool row_ok = a < a1;
    const int64_t ia = row_ok ? (A.F.idx ? A.F.idx[a] : a) : 0;
    const int pf_i = row_ok ? A.F.pos[ia] : 0;
    {   // the extremes: rows by wave 0, columns by all (SS_C == SS_THREADS)
        int mn = 0x7FFFFFFF, mx = (int)0x80000000;
        if (w == 0 && row_ok) mn = mx = pf_i;
        int tn = 0x7FFFFFFF, tx = (int)0x80000000;
        if (b0 + tid < b1) s_pt[tid] = tn = tx = A.T.pos[A.T.idx ? A.T.idx[b0 + tid] : b0 + tid];
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
    // x = pos1 - pos2 (to side - from side) of the patch lies in [x0, x1]; len(x) is the triangle wave of period g (k_decay_hist)
    const double g = A.g, x0 = (double)s_ext[2] - (double)s_ext[1], x1 = (double)s_ext[3] - (double)s_ext[0];
    double lmin = 0.0, lmax = 0.5 * g;
    if (x1 - x0 < g) {
        const double l0 = circ_len(x0, 0.0, g), l1 = circ_len(x1, 0.0, g);
        if (floor(x1 / g) == floor(x0 / g)) lmin = fmin(l0, l1);
        if (floor((x1 - 0.5 * g) / g) == floor((x0 - 0.5 * g) / g)) lmax = fmax(l0, l1);
    }
    const int P = lmax <= A.sr_dist ? 0 : (lmin > A.sr_dist ? 1 : -1);   // the class of the whole patch; -1: the bound does not say
    if (A.route == 1 && P < 0) {
        if (tid == 0) atomicAdd(&A.stat[4], 1ull);
        return;
    }
    const bool single = P >= 0 && A.route != 2;
    if (tid == 0) {
        atomicAdd(&A.stat[0], 1ull);
        if (!single) atomicAdd(&A.stat[1], 1ull);
    }
    uint32_t rn[2], rg[2], refused = 0;
    long long rs[2];
    unsigned long long rm[2];
    unsigned long long *tile = s_tile + w * (SS_B * SS_LD);
    if (single) ss_columns<1>(A, P, tile, s_pt, a, a1, row_ok, (double)pf_i, b0, b1, lane, w, rn, rs, rm, rg, refused);
    else ss_columns<2>(A, 0, tile, s_pt, a, a1, row_ok, (double)pf_i, b0, b1, lane, w, rn, rs, rm, rg, refused);
    for (int o = 32; o; o >>= 1) refused += __shfl_xor(refused, o);
    if (lane == 0 && refused) atomicAdd(&A.stat[3], (unsigned long long)refused);
    // the four waves' row sums through LDS: value k = quantity * 2 + class of wave v and row r at (v * 8 + k) * 64 + r
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        s_tile[(w * 8 + 0 + c) * 64 + lane] = rn[c];
        s_tile[(w * 8 + 2 + c) * 64 + lane] = (unsigned long long)rs[c];
        s_tile[(w * 8 + 4 + c) * 64 + lane] = rm[c];
        s_tile[(w * 8 + 6 + c) * 64 + lane] = rg[c];
    }
    __syncthreads();
    // wave w combines quantity w of both classes
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int k = w * 2 + c;
        unsigned long long t = 0;
#pragma unroll
        for (int v = 0; v < SS_WAVES; ++v) {
            const unsigned long long x = s_tile[(v * 8 + k) * 64 + lane];
            t = w == 2 ? (x > t ? x : t) : t + x;
        }
        if (row_ok && t) {
            if (w == 2) ss_max(A.F.at(2, c, ia), t);
            else ss_add(A.F.at(w, c, ia), t);
        }
        if (w == 0) {   // the pairs of the class: the partners of the patch's rows
            unsigned long long np = t;
            for (int o = 32; o; o >>= 1) np += __shfl_xor(np, o);
            if (lane == 0 && np) atomicAdd(&A.stat[5 + c], np);
        }
    }
}

constexpr int SS_NSTAT = 8;

// One summary: the device-side accumulators and counters
struct SnpSumRun {
    DevBuf accF, accT, stat;
    int64_t lenF = 0, lenT = 0;
    bool shared = false;   // both sides add to accF (the SNPs of an alignment); else rows to accF, columns to accT (the debug entry)
};

static size_t ss_bytes(int64_t len) { return (size_t)SS_NQ * 2 * (size_t)len * 8; }

static int snpsum_check(double sr_dist, const double *thr, const char *who) {
    LDW_REQUIRE(thr, LDW_ERR_ARG, "%s: null thr", who);
    LDW_REQUIRE(!std::isnan(sr_dist) && sr_dist >= 0, LDW_ERR_ARG, "%s: sr_dist must be a non-negative number (+inf allowed)", who);
    return LDW_OK;
}

static int snpsum_begin(ldw_ctx *c, SnpSumRun &R, int64_t lenF, int64_t lenT, bool shared) {
    R.lenF = lenF, R.lenT = shared ? lenF : lenT, R.shared = shared;
    if (int rc = R.accF.reserve(ss_bytes(R.lenF))) return rc;
    LDW_HIP(hipMemsetAsync(R.accF.p, 0, ss_bytes(R.lenF), c->stream));
    if (!shared) {
        if (int rc = R.accT.reserve(ss_bytes(R.lenT))) return rc;
        LDW_HIP(hipMemsetAsync(R.accT.p, 0, ss_bytes(R.lenT), c->stream));
    }
    if (int rc = R.stat.reserve(SS_NSTAT * 8)) return rc;
    LDW_HIP(hipMemsetAsync(R.stat.p, 0, SS_NSTAT * 8, c->stream));
    return LDW_OK;
}

static int snpsum_launch(ldw_ctx *c, const SnpSumRun &R, const double *MI, int64_t nf, int64_t nt, const int32_t *pos_f, const int32_t *idx_f, const int32_t *pos_t,
                         const int32_t *idx_t, double g, int diag, double sr_dist, const double *thr, int route) {
    SnpSumArgs A;
    A.MI = MI, A.nf = nf, A.nt = nt;
    A.F.acc = R.accF.as<unsigned long long>(), A.F.len = R.lenF, A.F.pos = pos_f, A.F.idx = idx_f;
    A.T.acc = (R.shared ? R.accF : R.accT).as<unsigned long long>(), A.T.len = R.lenT, A.T.pos = pos_t, A.T.idx = idx_t;
    A.g = g, A.sr_dist = sr_dist, A.thr0 = thr[0], A.thr1 = thr[1], A.diag = diag, A.route = route;
    A.stat = R.stat.as<unsigned long long>();
    const dim3 grid((unsigned)((nf + SS_ROWS - 1) / SS_ROWS), (unsigned)((nt + SS_C - 1) / SS_C));
    hipLaunchKernelGGL(k_snp_summary, grid, dim3(SS_THREADS), 0, c->stream, A);
    LDW_HIP(hipGetLastError());
    return LDW_OK;
}

// one side's accumulators to the host (max_out and nge_out may be null); then the stream is NOT yet synchronised: keys must outlive the copy
static int snpsum_fetch(ldw_ctx *c, const DevBuf &acc, int64_t len, int64_t *n_out, int64_t *sumq_out, std::vector<unsigned long long> &keys, bool want_max, int64_t *nge_out) {
    const size_t sec = 2 * (size_t)len * 8;
    const uint8_t *p = acc.as<uint8_t>();
    LDW_HIP(hipMemcpyAsync(n_out, p, sec, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemcpyAsync(sumq_out, p + sec, sec, hipMemcpyDeviceToHost, c->stream));
    if (want_max) {
        keys.resize(2 * (size_t)len);
        LDW_HIP(hipMemcpyAsync(keys.data(), p + 2 * sec, sec, hipMemcpyDeviceToHost, c->stream));
    }
    if (nge_out) LDW_HIP(hipMemcpyAsync(nge_out, p + 3 * sec, sec, hipMemcpyDeviceToHost, c->stream));
    return LDW_OK;
}

// the largest value of every (class, SNP) from its key: NaN where the SNP has no partner of the class
static void snpsum_max(const std::vector<unsigned long long> &keys, const int64_t *n, double *max_out) {
    for (size_t k = 0; k < keys.size(); ++k) max_out[k] = n[k] ? key_f64(keys[k]) : std::nan("");
}

}  // namespace ldw

extern "C" {

int ldw_mi_snp_summary(ldw_ctx *c, const int32_t *blocks, int64_t nblocks, int quirk_mode, double sr_dist, const double *thr, int64_t *n_out, int64_t *sumq_out,
                       double *max_out, int64_t *nge_out, int64_t *npairs_out) {
    if (int rc = pair_blocks_check(c, "ldw_mi_snp_summary", blocks, nblocks, quirk_mode, n_out && sumq_out && npairs_out,
                                   [&] { return snpsum_check(sr_dist, thr, "ldw_mi_snp_summary"); }))
        return rc;
    SnpSumRun R;
    if (int rc = snpsum_begin(c, R, c->L, c->L, true)) return rc;
    PairBlockWalk W;
    if (int rc = pair_blocks_walk(c, blocks, nblocks, quirk_mode, W, [&](int64_t nf, int64_t nt, bool diag) {
            return snpsum_launch(c, R, c->MIblk.as<double>(), nf, nt, c->meta.POS.as<int32_t>(), c->idx_f.as<int32_t>(), c->meta.POS.as<int32_t>(), c->idx_t.as<int32_t>(),
                                 c->meta.g, diag ? 1 : 0, sr_dist, thr, 0);
        }))
        return rc;
    std::vector<unsigned long long> keys;
    unsigned long long st[SS_NSTAT];
    if (int rc = snpsum_fetch(c, R.accF, c->L, n_out, sumq_out, keys, max_out != nullptr, nge_out)) return rc;
    LDW_HIP(hipMemcpyAsync(st, R.stat.p, sizeof st, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    if (max_out) snpsum_max(keys, n_out, max_out);
    npairs_out[0] = (int64_t)st[5], npairs_out[1] = (int64_t)st[6];
    LDW_REQUIRE(npairs_out[0] + npairs_out[1] == W.npairs, LDW_ERR_STATE, "ldw_mi_snp_summary: %lld + %lld pairs counted, %lld visited", (long long)npairs_out[0],
                (long long)npairs_out[1], (long long)W.npairs);
    for (int k = 0; k < 4; ++k) c->snpsum_stat[k] = (int64_t)st[k];
    c->snpsum_stat[4] = nblocks;
    c->last_ms[0] = W.ms_mi, c->last_ms[1] = W.ms_consumer, c->last_ms[2] = 0, c->last_ms[3] = W.ms_mi + W.ms_consumer;
    return LDW_OK;
}

int ldw_snp_summary_report(ldw_ctx *c, int64_t out[5]) {
    LDW_REQUIRE(c && out, LDW_ERR_ARG, "ldw_snp_summary_report: null argument");
    for (int k = 0; k < 5; ++k) out[k] = c->snpsum_stat[k];
    return LDW_OK;
}

int ldw_debug_snp_summary(ldw_ctx *c, const double *mi, int64_t nf, int64_t nt, const int32_t *pos_f, const int32_t *pos_t, double g, int diag, double sr_dist,
                          const double *thr, int route, int64_t *n_f, int64_t *sumq_f, double *max_f, int64_t *nge_f, int64_t *n_t, int64_t *sumq_t, double *max_t,
                          int64_t *nge_t, int64_t *npairs_out, int64_t *stats_out) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(mi && pos_f && pos_t && n_f && sumq_f && n_t && sumq_t && npairs_out, LDW_ERR_ARG, "ldw_debug_snp_summary: null argument");
    LDW_REQUIRE(nf >= 1 && nt >= 1 && nf <= 1000000 && nt <= 1000000, LDW_ERR_ARG, "ldw_debug_snp_summary: nf, nt outside 1..1 000 000");
    LDW_REQUIRE(diag == 0 || (diag == 1 && nf == nt), LDW_ERR_ARG, "ldw_debug_snp_summary: diag is 0 or 1, and a diagonal block is square");
    LDW_REQUIRE(std::isfinite(g) && g > 0, LDW_ERR_ARG, "ldw_debug_snp_summary: g must be positive");
    LDW_REQUIRE(route >= 0 && route <= 2, LDW_ERR_ARG, "ldw_debug_snp_summary: route outside 0..2");
    if (int rc = snpsum_check(sr_dist, thr, "ldw_debug_snp_summary")) return rc;
    if (int rc = join_prepare(c)) return rc;
    SnpSumRun R;
    DevBuf d_mi, d_pf, d_pt;
    if (int rc = snpsum_begin(c, R, nf, nt, false)) return rc;
    if (int rc = upload(c, d_mi, mi, (size_t)(nf * nt))) return rc;
    if (int rc = upload(c, d_pf, pos_f, (size_t)nf)) return rc;
    if (int rc = upload(c, d_pt, pos_t, (size_t)nt)) return rc;
    if (int rc = snpsum_launch(c, R, d_mi.as<double>(), nf, nt, d_pf.as<int32_t>(), nullptr, d_pt.as<int32_t>(), nullptr, g, diag, sr_dist, thr, route)) return rc;
    std::vector<unsigned long long> keys_f, keys_t;
    unsigned long long st[SS_NSTAT];
    if (int rc = snpsum_fetch(c, R.accF, nf, n_f, sumq_f, keys_f, max_f != nullptr, nge_f)) return rc;
    if (int rc = snpsum_fetch(c, R.accT, nt, n_t, sumq_t, keys_t, max_t != nullptr, nge_t)) return rc;
    LDW_HIP(hipMemcpyAsync(st, R.stat.p, sizeof st, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    LDW_REQUIRE(st[4] == 0, LDW_ERR_ARG, "ldw_debug_snp_summary: route 1, but the bound of %llu patches does not put them in one class", st[4]);
    if (max_f) snpsum_max(keys_f, n_f, max_f);
    if (max_t) snpsum_max(keys_t, n_t, max_t);
    npairs_out[0] = (int64_t)st[5], npairs_out[1] = (int64_t)st[6];
    if (stats_out)
        for (int k = 0; k < 4; ++k) stats_out[k] = (int64_t)st[k];
    return LDW_OK;
}

}  // extern "C"
