// The permutation test for links, within lineages (include/ldweaver_amd.h 19): ldw_links_permuted gives, per listed SNP pair, the weighted MI
// over all labelled sequences, and how many of B replicates reach it when SNP b's states are permuted among the sequences of every cluster.
//
// Orders.  order0[P] is the labelled sequences by (label, sequence).  Replicates go in batches of R <= 256:
//   k_perm_keys   item (r, p) of the batch: key (r << 56) | (label << 40) | h(seed, r0 + r, order0[p]), value order0[p];
//   one stable radix sort of the R P items (ldw_prim.h) leaves order_r[p], replicate after replicate.
// Pairs.
//   k_perm_pairs  a workgroup per (pair, group of replicates of the batch).  The prologue stages into LDS SNP b's row of the states by sequence and SNP a's
//                 states in order0 order, both clamped to 0..4, and, where they still fit, the weights V in order0 order; the masks of the states either
//                 SNP shows among the labelled sequences and the sums of V by a's state come out of the same pass.  A wave takes whole replicates:
//                 lane l walks p = l, l + 64, ..., reads order_r[p] coalesced, gathers b's byte from LDS and adds V[p] to the cell (a's state, b's
//                 state) — only the cells of the states the two SNPs show at all, wave-uniform branches on the two masks with static register indices,
//                 as lin_walk has them.  What no replicate changes is not recomputed: the count marginals (the states present are the two masks) and
//                 a's sums of V (the column of b's last state is a's sum less the other columns).  A shuffle reduction and lin_eval
//                 (ldw_lin_table.h) on lane 0 close the replicate.  The observed value is the same kernel on order0.
//   k_perm_count  a wave per pair: the batch's replicates with mi_r >= mi_obs added to the count, the largest to the maximum.  Integer sums and maxima:
//                 nothing depends on how replicates or pairs are batched.
#pragma clang fp contract(off)
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "ldw_internal.h"
#include "ldw_lin_table.h"
#include "ldw_prim.h"
#include "ldw_seq_plan.h"   // LabelSet, perm_order0, budget_or_env: the host side of ldw_links_permuted

using namespace ldw;

namespace ldw {

constexpr int PERM_MAX_BATCH = 256;                     // replicates per sort: the batch-local replicate takes the key's top 8 bits
constexpr int64_t PERM_BUDGET = (int64_t)1 << 30;       // bytes the keys, values and sort storage of a batch may take; and, apart, the outputs of a chunk of pairs
constexpr int PERM_MAX_CLUSTERS = 65536;                // the label takes 16 bits of the key
constexpr int PERM_MAX_REPLICATES = 1 << 24;
constexpr int PERM_THREADS = 512;                       // 8 waves: two per SIMD where the staged rows leave room for one workgroup per CU only
constexpr int PERM_WAVES = PERM_THREADS / 64;
constexpr int PERM_UNROLL = 4;                          // positions a lane takes per step of a replicate
constexpr int64_t PERM_LDS_MAX = 160 * 1024;            // LDS of a CU
constexpr int64_t PERM_LDS_HEAD = 64;                   // in front of the staged arrays: the two masks, then at byte 16 the five sums of V by a's state
constexpr int64_t PERM_LDS_WITH_V = 80 * 1024;          // V goes to LDS too while two workgroups still fit a CU

// the 40-bit hash of (seed, replicate, sequence): include/ldweaver_amd.h (19)
__host__ __device__ __forceinline__ uint64_t perm_hash(uint64_t seed, uint64_t r, uint64_t s) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (r + 1) + 0xD1B54A32D192ED03ull * (s + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z >> 24;
}

// items [0, R P): key[r P + p] = (r << 56) | (label << 40) | h(seed, r0 + r, s), val = s, with s = order0[p]
__global__ __launch_bounds__(256) void k_perm_keys(const int32_t *__restrict__ order0, const int32_t *__restrict__ labels, int64_t P, int64_t R, int64_t r0, uint64_t seed,
                                                   uint64_t *__restrict__ key, int32_t *__restrict__ val) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= R * P) return;
    const int64_t r = i / P, p = i - r * P;
    const int32_t s = order0[p];
    key[i] = ((uint64_t)r << 56) | ((uint64_t)(uint32_t)labels[s] << 40) | perm_hash(seed, (uint64_t)(r0 + r), (uint64_t)s);
    val[i] = s;
}

__device__ __forceinline__ uint32_t perm_clamp(uint32_t raw) { return raw < 4u ? raw : 4u; }

// MODE 0: V, b's row and a's states in LDS; 1: the two state arrays in LDS, V read from global memory; 2: nothing staged (more sequences than LDS holds):
// the states are gathered from global memory.  Dynamic LDS: [the two masks, PERM_LDS_HEAD bytes] [V int64 [P] (MODE 0)] [b's row, Npad bytes] [a's states in order0 order, P bytes].
// grid (pairs of the chunk, groups of G replicates); orders[R][P]; mi[k * ld + r]; fix[(k * ld + r) * 25 + cell] (may be null).
template <int MODE>
__global__ __launch_bounds__(PERM_THREADS) void k_perm_pairs(const uint8_t *__restrict__ states, int64_t Npad, const int32_t *__restrict__ pair_a, const int32_t *__restrict__ pair_b,
                                                             const int32_t *__restrict__ order0, const int64_t *__restrict__ v0, const int32_t *__restrict__ orders,
                                                             int64_t P, int32_t R, int32_t G, double neff, double scale, int64_t ld,
                                                             double *__restrict__ mi, int64_t *__restrict__ fix) {
    extern __shared__ __align__(16) uint8_t perm_lds[];
    uint32_t *s_mask = reinterpret_cast<uint32_t *>(perm_lds);   // (in the dynamic block: with a static one beside it the kernel could not ask for all 160 KiB)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t k = blockIdx.x;
    const uint8_t *__restrict__ row_a = states + (int64_t)pair_a[k] * Npad, *__restrict__ row_b = states + (int64_t)pair_b[k] * Npad;
    int64_t *lds_v = reinterpret_cast<int64_t *>(perm_lds + PERM_LDS_HEAD);
    uint8_t *lds_b = perm_lds + PERM_LDS_HEAD + (MODE == 0 ? P * 8 : 0), *lds_a = lds_b + Npad;

    // ---- prologue: the masks of the states seen among the labelled sequences; the staged arrays ----
    unsigned long long *s_fa = reinterpret_cast<unsigned long long *>(perm_lds + 16);
    if (tid < PERM_LDS_HEAD / 4) s_mask[tid] = 0;
    __syncthreads();
    uint32_t ma = 0, mb = 0;
    int64_t fa[5] = {0, 0, 0, 0, 0};   // the sum of V over the positions where a shows X: the same in every replicate, since V stays with a
    for (int64_t p = tid; p < P; p += PERM_THREADS) {
        const int32_t s = order0[p];
        const uint32_t x = perm_clamp(row_a[s]);
        const int64_t v = v0[p];
        ma |= 1u << x, mb |= 1u << perm_clamp(row_b[s]);
#pragma unroll
        for (int X = 0; X < 5; ++X) fa[X] += x == (uint32_t)X ? v : (int64_t)0;
        if (MODE <= 1) lds_a[p] = (uint8_t)x;
        if (MODE == 0) lds_v[p] = v;
    }
    if (MODE <= 1) {   // b's row by sequence, a word at a time (the row starts at a multiple of 128 bytes and Npad is one)
        const uint32_t *__restrict__ src = reinterpret_cast<const uint32_t *>(row_b);
        uint32_t *dst = reinterpret_cast<uint32_t *>(lds_b);
        for (int64_t w = tid; w < Npad / 4; w += PERM_THREADS) {
            const uint32_t x = src[w];
            dst[w] = perm_clamp(x & 255u) | (perm_clamp((x >> 8) & 255u) << 8) | (perm_clamp((x >> 16) & 255u) << 16) | (perm_clamp(x >> 24) << 24);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ma |= __shfl_xor(ma, off), mb |= __shfl_xor(mb, off);
#pragma unroll
    for (int X = 0; X < 5; ++X)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) fa[X] += (int64_t)__shfl_down((long long)fa[X], off);
    if (lane == 0) {
        atomicOr(&s_mask[0], ma), atomicOr(&s_mask[1], mb);
#pragma unroll
        for (int X = 0; X < 5; ++X) atomicAdd(&s_fa[X], (unsigned long long)fa[X]);
    }
    __syncthreads();
    const uint32_t pa = __builtin_amdgcn_readfirstlane(s_mask[0]), pb = __builtin_amdgcn_readfirstlane(s_mask[1]);

    // ---- the replicates of this group, a wave each ----
    // The count marginals of a replicate's table are the observed table's — a's states stay, b's are only reordered among the labelled sequences — so the
    // states present are the two masks, and lin_eval asks no more of the counts: it gets the table with a 1 wherever both states are present.
    LinTable t;
#pragma unroll
    for (int X = 0; X < 5; ++X)
#pragma unroll
        for (int Y = 0; Y < 5; ++Y) t.cnt[X * 5 + Y] = (int32_t)((pa >> X) & (pb >> Y) & 1u);
    // Nor does the loop visit the last of b's states: every position falls into one cell of its row, so that column is a's sums less the others.
    const int y_last = 31 - __builtin_clz(pb);
    const int32_t Pi = (int32_t)P;   // (P <= N < 2^31)
    const int32_t r_end = min(R, (int32_t)(blockIdx.y + 1) * G);
    for (int32_t r = (int32_t)blockIdx.y * G + __builtin_amdgcn_readfirstlane(wave); r < r_end; r += PERM_WAVES) {
        const int32_t *__restrict__ ord = orders + (int64_t)r * P;
#pragma unroll
        for (int q = 0; q < 25; ++q) t.fix[q] = 0;
        // PERM_UNROLL positions per lane and step: their loads are in flight together, and the walk over the masks is paid once for all of them
        for (int32_t p0 = lane; p0 < Pi; p0 += 64 * PERM_UNROLL) {
            uint32_t cell[PERM_UNROLL];
            int64_t v[PERM_UNROLL];
#pragma unroll
            for (int j = 0; j < PERM_UNROLL; ++j) {
                const int32_t p = p0 + 64 * j;
                cell[j] = 255u, v[j] = 0;   // past the last position: no cell
                if (p < Pi) {
                    const int32_t s = ord[p];
                    const uint32_t x = MODE <= 1 ? (uint32_t)lds_a[p] : perm_clamp(row_a[order0[p]]);
                    const uint32_t y = MODE <= 1 ? (uint32_t)lds_b[s] : perm_clamp(row_b[s]);
                    v[j] = MODE == 0 ? lds_v[p] : v0[p];
                    cell[j] = x * 5u + y;
                }
            }
#pragma unroll
            for (int X = 0; X < 5; ++X) {
                if (!((pa >> X) & 1u)) continue;
#pragma unroll
                for (int Y = 0; Y < 5; ++Y) {
                    if (!((pb >> Y) & 1u) || Y == y_last) continue;
#pragma unroll
                    for (int j = 0; j < PERM_UNROLL; ++j) t.fix[X * 5 + Y] += cell[j] == (uint32_t)(X * 5 + Y) ? v[j] : (int64_t)0;
                }
            }
        }
#pragma unroll
        for (int X = 0; X < 5; ++X) {   // lane 0 gets the wave's sums of the cells both SNPs can fill
            if (!((pa >> X) & 1u)) continue;
#pragma unroll
            for (int Y = 0; Y < 5; ++Y) {
                if (!((pb >> Y) & 1u) || Y == y_last) continue;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) t.fix[X * 5 + Y] += (int64_t)__shfl_down((long long)t.fix[X * 5 + Y], off);
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int X = 0; X < 5; ++X) {
                if (!((pa >> X) & 1u)) continue;
                int64_t rest = (int64_t)s_fa[X];
#pragma unroll
                for (int Y = 0; Y < 5; ++Y)
                    if (Y != y_last) rest -= t.fix[X * 5 + Y];
#pragma unroll
                for (int Y = 0; Y < 5; ++Y)
                    if (Y == y_last) t.fix[X * 5 + Y] = rest;
            }
            uint32_t pl = 0;
            const int64_t o = k * ld + r;
            mi[o] = lin_eval(t, scale, neff, &pl);
            if (fix) {
#pragma unroll
                for (int q = 0; q < 25; ++q) fix[o * 25 + q] = t.fix[q];
            }
        }
    }
}

// a wave per pair of the chunk: n_ge[k] += #{r < R: mi[k][r] >= obs[k]}, mx[k] = max(mx[k], max_r mi[k][r])
__global__ __launch_bounds__(256) void k_perm_count(const double *__restrict__ mi, int64_t ld, int32_t R, int64_t K, const double *__restrict__ obs, int32_t *__restrict__ n_ge,
                                                    double *__restrict__ mx) {
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= K) return;
    const double o = obs[k];
    int32_t n = 0;
    double m = -INFINITY;
    for (int32_t r = lane; r < R; r += 64) {
        const double v = mi[k * ld + r];
        n += v >= o ? 1 : 0;
        m = v > m ? v : m;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n += __shfl_xor(n, off);
        const double x = __shfl_xor(m, off);
        m = x > m ? x : m;
    }
    if (lane == 0) {
        n_ge[k] += n;
        mx[k] = m > mx[k] ? m : mx[k];
    }
}

__global__ __launch_bounds__(256) void k_perm_init(int64_t K, int32_t *__restrict__ n_ge, double *__restrict__ mx) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < K) n_ge[k] = 0, mx[k] = -INFINITY;
}

}  // namespace ldw

namespace {

struct PermBufs {   // the working memory of one ldw_links_permuted call
    ldw::DevBuf order0, labels, v0, pair_a, pair_b, key, key2, val, val2, sort, obs, n_ge, mx, mi, fix;
};

struct PermLaunch {   // what every launch of k_perm_pairs of a call shares
    int mode = 0;
    size_t lds = 0;
    int64_t P = 0;
    double neff = 0, scale = 1;
};

// pairs [k0, k0 + kc) on the R replicates whose orders are at `orders`; G replicates per workgroup
int launch_pairs(ldw_ctx *c, const PermBufs &b, const PermLaunch &pl, int64_t k0, int64_t kc, const int32_t *orders, int32_t R, int64_t ld, double *mi, int64_t *fix) {
    // enough workgroups for every CU twice over, a workgroup's replicates a multiple of its waves: the prologue is shared by all of them
    const int64_t want = std::max<int64_t>(1, ceil_div(2 * (int64_t)std::max(c->n_cu, 1), kc));
    const int64_t groups = std::min<int64_t>(want, ceil_div(R, PERM_WAVES));
    const int32_t G = (int32_t)(ceil_div(ceil_div(R, groups), PERM_WAVES) * PERM_WAVES);
    const dim3 grid((unsigned)kc, (unsigned)ceil_div(R, G)), block(PERM_THREADS);
    const int32_t *pa = b.pair_a.as<int32_t>() + k0, *pb = b.pair_b.as<int32_t>() + k0;
#define LDW_PERM_LAUNCH(M)                                                                                                                                          \
    hipLaunchKernelGGL(k_perm_pairs<M>, grid, block, pl.lds, c->stream, c->states.as<uint8_t>(), c->Npad, pa, pb, b.order0.as<int32_t>(), b.v0.as<int64_t>(), orders, \
                       pl.P, R, G, pl.neff, pl.scale, ld, mi, fix)
    if (pl.mode == 0) LDW_PERM_LAUNCH(0);
    else if (pl.mode == 1) LDW_PERM_LAUNCH(1);
    else LDW_PERM_LAUNCH(2);
#undef LDW_PERM_LAUNCH
    LDW_HIP(hipGetLastError());
    return LDW_OK;
}

int permuted_run(ldw_ctx *c, const int32_t *pair_a, const int32_t *pair_b, int64_t K, const int32_t *labels, int32_t C, int32_t B, uint64_t seed, double *mi_obs_out,
                 int32_t *n_ge_out, double *null_max_out, double *null_out, int64_t *fixed_out, int32_t *order_out, int64_t *p_out, int *frac_bits_out, PermBufs &b) {
    const char *who = "ldw_links_permuted";
    LDW_REQUIRE(ldw::have_alignment(c), LDW_ERR_STATE, "%s: no alignment resident: set the alignment first", who);
    LDW_REQUIRE(c->wts.have_weights, LDW_ERR_STATE, "%s: no weights resident: set the weights first", who);
    LDW_REQUIRE(pair_a && pair_b && labels, LDW_ERR_ARG, "%s: pair_a, pair_b or labels is null", who);
    LDW_REQUIRE(mi_obs_out && n_ge_out && null_max_out && p_out && frac_bits_out, LDW_ERR_ARG, "%s: a required output is null", who);
    LDW_REQUIRE(K >= 1, LDW_ERR_ARG, "%s: %lld pairs (at least 1)", who, (long long)K);
    LDW_REQUIRE(K < (1ll << 31), LDW_ERR_ARG, "%s: too many pairs", who);
    LDW_REQUIRE(B >= 1 && B <= PERM_MAX_REPLICATES, LDW_ERR_ARG, "%s: B = %d replicates (1..%d)", who, (int)B, PERM_MAX_REPLICATES);
    LDW_REQUIRE(C >= 1 && C <= PERM_MAX_CLUSTERS, LDW_ERR_ARG, "%s: C = %d clusters (1..%d)", who, (int)C, PERM_MAX_CLUSTERS);
    const int64_t N = c->N, L = c->L, Npad = c->Npad;
    const ldw::LabelSet ls = ldw::LabelSet::scan(labels, N, C);
    LDW_REQUIRE(ls.bad < 0, LDW_ERR_ARG, "%s: labels[%lld] = %d (-1, or a cluster 0..%d)", who, (long long)ls.bad, (int)labels[ls.bad], (int)(C - 1));
    const int64_t P = ls.P;
    LDW_REQUIRE(P >= 1, LDW_ERR_ARG, "%s: every label is -1: no sequence to permute", who);
    int64_t bad_k = -1;
    const int32_t *bad = ldw::first_bad_pair(pair_a, pair_b, K, L, &bad_k);
    LDW_REQUIRE(!bad, LDW_ERR_ARG, "%s: %s[%lld] = %d (the alignment has SNPs 0..%lld)", who, bad == pair_a ? "pair_a" : "pair_b", (long long)bad_k, (int)bad[bad_k], (long long)(L - 1));
    const std::vector<int64_t> &V = c->wts.h_vfixed;
    const std::vector<double> &hdw = c->wts.h_hdw;

    // ---- order0: the labelled sequences by (label, sequence) and the weights in that order (ldw_seq_plan.h); neff as mi_all has it ----
    const ldw::PermOrder po = ldw::perm_order0(labels, V.data(), N, C);
    std::vector<double> neff((size_t)C + 1);
    ldw::LabelSet::neff(labels, hdw.data(), N, C, neff.data());
    PermLaunch pl;
    pl.P = P;
    pl.neff = neff[(size_t)C];
    pl.scale = std::ldexp(1.0, -c->wts.frac_bits);

    // ---- what goes to LDS.  LDW_PERM_LDS=m in the environment asks for mode m or, where that does not fit, the next that does: a test hook ----
    const int64_t lds_states = PERM_LDS_HEAD + Npad + ceil_div(P, 16) * 16;
    pl.mode = P * 8 + lds_states <= PERM_LDS_WITH_V ? 0 : lds_states <= PERM_LDS_MAX ? 1 : 2;
    if (const long long m = ldw::env_int("LDW_PERM_LDS"); m >= 0 && m <= 2) pl.mode = std::max(pl.mode, (int)m);   // (the hook's own rule: only the read is shared)
    pl.lds = pl.mode == 0 ? (size_t)(P * 8 + lds_states) : pl.mode == 1 ? (size_t)lds_states : (size_t)PERM_LDS_HEAD;
    if (pl.lds > 64 * 1024) {   // past what a kernel gets without asking
        const void *fn = pl.mode == 0 ? reinterpret_cast<const void *>(k_perm_pairs<0>) : reinterpret_cast<const void *>(k_perm_pairs<1>);
        LDW_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PERM_LDS_MAX));
    }

    // ---- replicates per batch: keys and values twice over and the sort's storage within the budget.  LDW_PERM_BATCH=k forces k: a test hook ----
    const bool forced = ldw::env_int("LDW_PERM_BATCH") >= 1;
    int64_t R = ldw::budget_or_env(std::max<int64_t>(1, PERM_BUDGET / (P * 40)), "LDW_PERM_BATCH");
    R = std::min<int64_t>(std::min<int64_t>(R, PERM_MAX_BATCH), B);
    const unsigned end_bit = 56 + 8;
    size_t sort_bytes = 0;
    for (;;) {   // (the sort's storage is known only once asked for: halve R while it does not fit)
        LDW_HIP((ldw::prim_sort_pairs_bytes<uint64_t, int32_t>((size_t)(R * P), 0, end_bit, c->stream, &sort_bytes)));
        if (R == 1 || forced || (int64_t)sort_bytes + R * P * 24 <= PERM_BUDGET) break;
        R /= 2;
    }
    const int64_t R_tail = B % R;
    size_t sort_bytes_tail = 0;
    if (R_tail) LDW_HIP((ldw::prim_sort_pairs_bytes<uint64_t, int32_t>((size_t)(R_tail * P), 0, end_bit, c->stream, &sort_bytes_tail)));

    // ---- pairs per chunk: a chunk's (pairs, R) values and, on request, tables within the budget.  LDW_PERM_CHUNK=k forces k: a test hook ----
    const int64_t cell_bytes = 8 + (fixed_out ? 200 : 0);
    const int64_t chunk = std::min<int64_t>(ldw::budget_or_env(std::max<int64_t>(1, PERM_BUDGET / (R * cell_bytes)), "LDW_PERM_CHUNK"), K);

    int rc = LDW_OK;
    const size_t items = (size_t)(R * P);
    if ((rc = ldw::upload(c, b.order0, po.order0.data(), po.order0.size())) || (rc = ldw::upload(c, b.v0, po.v0.data(), po.v0.size())) ||
        (rc = ldw::upload(c, b.labels, labels, (size_t)N)) || (rc = ldw::upload(c, b.pair_a, pair_a, (size_t)K)) || (rc = ldw::upload(c, b.pair_b, pair_b, (size_t)K)) ||
        (rc = b.key.reserve(items * 8)) || (rc = b.key2.reserve(items * 8)) || (rc = b.val.reserve(items * 4)) || (rc = b.val2.reserve(items * 4)) ||
        (rc = b.sort.reserve(std::max(sort_bytes, sort_bytes_tail) + 256)) || (rc = b.obs.reserve((size_t)K * 8)) || (rc = b.n_ge.reserve((size_t)K * 4)) ||
        (rc = b.mx.reserve((size_t)K * 8)) || (rc = b.mi.reserve((size_t)(chunk * R) * 8)) || (fixed_out && (rc = b.fix.reserve((size_t)(chunk * R) * 200))))
        return rc;
    ldw::Event ev[4];   // (no ldw::Laps: every step is timed as soon as its synchronisation returns, and the (batch, chunk) steps have no useful bound)
    for (ldw::Event &e : ev) LDW_HIP(e.ensure());
    double ms[3] = {0, 0, 0};   // the pair kernel (with the counts), keys and sorts, copies out
    auto lap = [&](int slot, int from) -> int {   // the time between ev[from] and ev[from + 1], once the stream has passed both
        float x = 0;
        LDW_HIP(hipEventElapsedTime(&x, ev[from], ev[from + 1]));
        ms[slot] += x;
        return LDW_OK;
    };

    // ---- the observed values: the same kernel on order0 as the one replicate ----
    LDW_HIP(hipEventRecord(ev[0], c->stream));
    hipLaunchKernelGGL(k_perm_init, dim3((unsigned)ceil_div(K, 256)), dim3(256), 0, c->stream, K, b.n_ge.as<int32_t>(), b.mx.as<double>());
    LDW_HIP(hipGetLastError());
    if ((rc = launch_pairs(c, b, pl, 0, K, b.order0.as<int32_t>(), 1, 1, b.obs.as<double>(), nullptr))) return rc;
    LDW_HIP(hipEventRecord(ev[1], c->stream));
    LDW_HIP(hipMemcpyAsync(mi_obs_out, b.obs.p, (size_t)K * 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipEventRecord(ev[2], c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    if ((rc = lap(0, 0)) || (rc = lap(2, 1))) return rc;

    for (int64_t r0 = 0; r0 < B; r0 += R) {
        const int32_t Rc = (int32_t)std::min<int64_t>(R, B - r0);
        const size_t n = (size_t)Rc * (size_t)P;
        size_t bytes = Rc == R ? sort_bytes : sort_bytes_tail;
        LDW_HIP(hipEventRecord(ev[0], c->stream));
        hipLaunchKernelGGL(k_perm_keys, dim3((unsigned)ceil_div((int64_t)n, 256)), dim3(256), 0, c->stream, b.order0.as<int32_t>(), b.labels.as<int32_t>(), P, (int64_t)Rc, r0,
                           seed, b.key.as<uint64_t>(), b.val.as<int32_t>());
        LDW_HIP(hipGetLastError());
        LDW_HIP((ldw::prim_sort_pairs<uint64_t, int32_t>(b.sort.p, bytes, b.key.as<uint64_t>(), b.key2.as<uint64_t>(), b.val.as<int32_t>(), b.val2.as<int32_t>(), n, 0, end_bit,
                                                        c->stream)));
        LDW_HIP(hipEventRecord(ev[1], c->stream));
        if (order_out) LDW_HIP(hipMemcpyAsync(order_out + r0 * P, b.val2.p, n * 4, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipEventRecord(ev[2], c->stream));
        LDW_HIP(hipStreamSynchronize(c->stream));
        if ((rc = lap(1, 0)) || (rc = lap(2, 1))) return rc;
        for (int64_t k0 = 0; k0 < K; k0 += chunk) {
            const int64_t kc = std::min<int64_t>(chunk, K - k0);
            LDW_HIP(hipEventRecord(ev[0], c->stream));
            if ((rc = launch_pairs(c, b, pl, k0, kc, b.val2.as<int32_t>(), Rc, Rc, b.mi.as<double>(), fixed_out ? b.fix.as<int64_t>() : nullptr))) return rc;
            hipLaunchKernelGGL(k_perm_count, dim3((unsigned)ceil_div(kc, 4)), dim3(256), 0, c->stream, b.mi.as<double>(), (int64_t)Rc, Rc, kc, b.obs.as<double>() + k0,
                               b.n_ge.as<int32_t>() + k0, b.mx.as<double>() + k0);
            LDW_HIP(hipGetLastError());
            LDW_HIP(hipEventRecord(ev[1], c->stream));
            if (null_out)   // rows of Rc values into rows of B
                LDW_HIP(hipMemcpy2DAsync(null_out + k0 * B + r0, (size_t)B * 8, b.mi.p, (size_t)Rc * 8, (size_t)Rc * 8, (size_t)kc, hipMemcpyDeviceToHost, c->stream));
            if (fixed_out)
                LDW_HIP(hipMemcpy2DAsync(fixed_out + (k0 * B + r0) * 25, (size_t)B * 200, b.fix.p, (size_t)Rc * 200, (size_t)Rc * 200, (size_t)kc, hipMemcpyDeviceToHost, c->stream));
            LDW_HIP(hipEventRecord(ev[2], c->stream));
            LDW_HIP(hipStreamSynchronize(c->stream));   // (the chunk's buffers are written again by the next)
            if ((rc = lap(0, 0)) || (rc = lap(2, 1))) return rc;
        }
    }
    LDW_HIP(hipEventRecord(ev[0], c->stream));
    LDW_HIP(hipMemcpyAsync(n_ge_out, b.n_ge.p, (size_t)K * 4, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemcpyAsync(null_max_out, b.mx.p, (size_t)K * 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipEventRecord(ev[1], c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    if ((rc = lap(2, 0))) return rc;
    *p_out = P;
    *frac_bits_out = c->wts.frac_bits;
    c->last_ms[0] = ms[0];
    c->last_ms[1] = ms[1];
    c->last_ms[2] = ms[2];
    c->last_ms[3] = ms[0] + ms[1] + ms[2];
    return LDW_OK;
}

}  // namespace

extern "C" int ldw_links_permuted(ldw_ctx *c, const int32_t *pair_a, const int32_t *pair_b, int64_t K, const int32_t *labels, int32_t C, int32_t B, uint64_t seed,
                                  double *mi_obs_out, int32_t *n_ge_out, double *null_max_out, double *null_out, int64_t *fixed_out, int32_t *order_out, int64_t *p_out,
                                  int *frac_bits_out) {
    return ldw::scoped_call<PermBufs>(c, [&](PermBufs &b) {
        return permuted_run(c, pair_a, pair_b, K, labels, C, B, seed, mi_obs_out, n_ge_out, null_max_out, null_out, fixed_out, order_out, p_out, frac_bits_out, b);
    });
}
