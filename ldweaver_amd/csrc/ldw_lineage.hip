// The lineage check for links: ldw_seq_clusters cuts the sequences into single-linkage clusters from the Hamming stage's exact shared-state
// counts; ldw_links_stratified gives, per cluster, the joint tables and the weighted MI of listed SNP pairs.
//
// Clusters.  G and scnt come from hamming_gram (ldw_hamming.h).  Per threshold t:
//   k_clu_adj    adj[i][w] bit b = [L - shared(i, 64 w + b) < t] (a wave per row and word, one ballot per threshold; bits past N are 0), up to 16
//                thresholds from one read of G;
//   k_clu_hook   a wave per vertex u: m = the smallest f over u's neighbours; where m < f[u], f[f[u]] and f[u] are lowered to m (atomicMin);
//   k_clu_jump   f[u] = f[f[u]], twice;
//                a round is the two of them, for every threshold that still moves at once (blockIdx.y); the host reads one word of "changed" bits back per
//                round and stops a threshold after its first round without a change: f[u] is then the smallest member of u's cluster (f only ever
//                falls, stays inside the cluster, and a round that changes nothing has f equal across every edge and f[f[u]] = f[u]);
//   k_clu_roots, an exclusive scan, k_clu_labels   clusters numbered in the order of their smallest member.
//
// Stratified tables.  The labelled sequences are ordered by (label, V, sequence); position p of that order is bit p & 63 of word p >> 6.  A maximal run of
// equal (label, V) is cut at word boundaries into PIECES (word, mask, V); a cluster is a range of pieces.
//   k_lin_bits   per distinct SNP of a chunk of pairs, five indicator bit rows over the positions (a wave per word: five ballots), and the SNP's mask of
//                states seen;
//   k_lin_pairs  a wave per pair walks the JOBS: a job is one large cluster, its pieces spread over the lanes and the 25 cells reduced over the wave, or
//                up to 64 small clusters, a lane each.  A cell is popc(row_a[X] & row_b[Y] & mask), added to an int32 count and, times V, to an int64
//                sum; only states the two SNPs show at all are visited.  The lane that holds a cluster's table evaluates its MI; every lane keeps the
//                sum of what it added, so the table over all labelled sequences costs one more reduction and evaluation at the end.
// Integers are exact and the evaluation of a table is one piece of code, so equal tables give equal bits.
#pragma clang fp contract(off)
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "ldw_internal.h"
#include "ldw_hamming.h"
#include "ldw_lin_table.h"   // LinTable, lin_eval, lin_zero, lin_add, lin_reduce: shared with ldw_perm.hip
#include "ldw_prim.h"
#include "ldw_seq_plan.h"   // LIN_SMALL, build_lin_plan, LabelSet, DistinctSlots: the host side of ldw_links_stratified

using namespace ldw;

namespace ldw {

constexpr int CLU_MAX_THRESH = 16;
constexpr int64_t CLU_ADJ_BYTES = (int64_t)2 << 30;   // the adjacency bits of the thresholds served by one read of G stay within this
constexpr int64_t LIN_BUDGET = (int64_t)1 << 30;      // bytes of working memory a chunk of pairs may take
constexpr int LIN_MAX_CLUSTERS = 65536;

struct CluThresh {
    int32_t n, t[CLU_MAX_THRESH];
};

// block: 4 rows of one word column; grid (ceil(N / 4), KW)
__global__ __launch_bounds__(256) void k_clu_adj(const int64_t *__restrict__ G, int ld, const int32_t *__restrict__ cnt, int64_t N, int64_t L, int64_t KW, CluThresh th,
                                                 uint64_t *__restrict__ adj) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), w = blockIdx.y, j = w * 64 + lane;
    if (i >= N) return;
    const int64_t d = j < N ? L - shared_ij(G, ld, cnt, L, i, j) : 0;
    uint64_t mine = 0;
    for (int g = 0; g < th.n; ++g) {
        const uint64_t m = __ballot(j < N && d < (int64_t)th.t[g]);
        if (lane == g) mine = m;
    }
    if (lane < th.n) adj[((int64_t)lane * N + i) * KW + w] = mine;
}

// f[g][u] = u
__global__ __launch_bounds__(256) void k_clu_init(int64_t N, int n_thresh, int32_t *__restrict__ f) {
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= N) return;
    for (int g = 0; g < n_thresh; ++g) f[(int64_t)g * N + u] = (int32_t)u;
}

// grid (ceil(N / 4), thresholds of the group); active: bit g = threshold g still moves
__global__ __launch_bounds__(256) void k_clu_hook(const uint64_t *__restrict__ adj, int64_t N, int64_t KW, uint32_t active, int32_t *f,
                                                  uint32_t *__restrict__ changed) {
    const int g = blockIdx.y, lane = threadIdx.x & 63;
    if (!((active >> g) & 1u)) return;
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= N) return;
    int32_t *fg = f + (int64_t)g * N;   // (read and lowered by other waves meanwhile: any value seen is a member of the cluster)
    const uint64_t *__restrict__ row = adj + ((int64_t)g * N + u) * KW;
    int32_t m = 0x7FFFFFFF;
    for (int64_t w = lane; w < KW; w += 64) {
        uint64_t x = row[w];
        while (x) {
            const int64_t v = w * 64 + __builtin_ctzll(x);   // (v < N: the bits past N are 0)
            x &= x - 1;
            const int32_t fv = fg[v];
            m = fv < m ? fv : m;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int32_t o = __shfl_xor(m, off);
        m = o < m ? o : m;
    }
    if (lane == 0) {
        const int32_t fu = fg[u];
        if (m < fu) {
            atomicMin(&fg[fu], m);
            atomicMin(&fg[u], m);
            atomicOr(changed, 1u << g);
        }
    }
}

// f[u] = f[f[u]], twice.  Only this thread writes f[u] here; what it reads of other vertices may be their old or their new value: both are members of the
// cluster not above the old one.
__global__ __launch_bounds__(256) void k_clu_jump(int64_t N, uint32_t active, int32_t *f, uint32_t *__restrict__ changed) {
    const int g = blockIdx.y;
    if (!((active >> g) & 1u)) return;
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= N) return;
    int32_t *fg = f + (int64_t)g * N;
    const int32_t f0 = fg[u];
    int32_t x = fg[f0];
    x = fg[x];
    if (x != f0) {
        fg[u] = x;
        atomicOr(changed, 1u << g);
    }
}

__global__ __launch_bounds__(256) void k_clu_roots(int64_t N, const int32_t *__restrict__ f, int32_t *__restrict__ is_root) {
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u <= N) is_root[u] = (u < N && f[u] == (int32_t)u) ? 1 : 0;   // (entry N: the scan's last one is the number of clusters)
}
__global__ __launch_bounds__(256) void k_clu_labels(int64_t N, const int32_t *__restrict__ f, const int32_t *__restrict__ rank, int32_t *__restrict__ label) {
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u < N) label[u] = rank[f[u]];
}

// ---- stratified tables ------------------------------------------------------------------------------------------------------------------------------

// grid (distinct SNPs of the chunk, ceil(W / 4)): a wave per 64-position word.  bits[(d * 5 + X) * W + w]; seen[d] bit X = state X occurs.
__global__ __launch_bounds__(256) void k_lin_bits(const uint8_t *__restrict__ states, int64_t Npad, const int32_t *__restrict__ snp, const int32_t *__restrict__ perm,
                                                  int64_t P, int64_t W, uint64_t *__restrict__ bits, uint32_t *__restrict__ seen) {
    const int lane = threadIdx.x & 63;
    const int64_t d = blockIdx.x, w = (int64_t)blockIdx.y * 4 + (threadIdx.x >> 6);
    if (w >= W) return;
    const int64_t p = w * 64 + lane;
    uint32_t st = 255;   // a position past the last one: no state
    if (p < P) {
        const uint32_t raw = states[(int64_t)snp[d] * Npad + perm[p]];
        st = raw < 4u ? raw : 4u;
    }
    uint64_t mine = 0;
#pragma unroll
    for (int X = 0; X < 5; ++X) {
        const uint64_t m = __ballot(st == (uint32_t)X);
        if (lane == X) mine = m;
    }
    if (lane < 5) {
        bits[(d * 5 + lane) * W + w] = mine;
        if (mine) atomicOr(&seen[d], 1u << lane);
    }
}

// the pieces [p0, p1) taken p0 + first, p0 + first + step, ...: their cells added to t
__device__ __forceinline__ void lin_walk(LinTable &t, const uint64_t *__restrict__ ra, const uint64_t *__restrict__ rb, int64_t W, uint32_t pa, uint32_t pb,
                                         const int32_t *__restrict__ pc_word, const uint64_t *__restrict__ pc_mask, const int64_t *__restrict__ pc_v, int64_t p0,
                                         int64_t p1, int first, int step) {
    for (int64_t p = p0 + first; p < p1; p += step) {
        const int64_t w = pc_word[p], V = pc_v[p];
        const uint64_t m = pc_mask[p];
        uint64_t A[5], B[5];
#pragma unroll
        for (int X = 0; X < 5; ++X) A[X] = ((pa >> X) & 1u) ? ra[X * W + w] & m : 0ull;
#pragma unroll
        for (int Y = 0; Y < 5; ++Y) B[Y] = ((pb >> Y) & 1u) ? rb[Y * W + w] : 0ull;
#pragma unroll
        for (int X = 0; X < 5; ++X) {
            if (!((pa >> X) & 1u)) continue;
#pragma unroll
            for (int Y = 0; Y < 5; ++Y) {
                if (!((pb >> Y) & 1u)) continue;
                const int32_t n = __popcll(A[X] & B[Y]);
                t.cnt[X * 5 + Y] += n;
                t.fix[X * 5 + Y] += V * (int64_t)n;
            }
        }
    }
}

// job j: job_count[j] == 0: the large cluster job_first[j], all lanes on its pieces; else lane l < job_count[j] takes the small cluster
// small[job_first[j] + l].  neff[C] is the sum over all labelled sequences.  Outputs of this chunk, zero where a cluster has no member:
// mi[k][C], poly[k][C], mi_all[k], tab_cnt / tab_fix [k][C][25] (may be null).
__global__ __launch_bounds__(256) void k_lin_pairs(const uint64_t *__restrict__ bits, const uint32_t *__restrict__ seen, int64_t W, const int32_t *__restrict__ slot_a,
                                                   const int32_t *__restrict__ slot_b, int64_t K, int32_t C, const int32_t *__restrict__ job_first,
                                                   const int32_t *__restrict__ job_count, int32_t n_jobs, const int32_t *__restrict__ small,
                                                   const int64_t *__restrict__ clu_piece, const int32_t *__restrict__ pc_word, const uint64_t *__restrict__ pc_mask,
                                                   const int64_t *__restrict__ pc_v, const double *__restrict__ neff, double scale, double *__restrict__ mi,
                                                   uint8_t *__restrict__ poly, double *__restrict__ mi_all, int64_t *__restrict__ tab_cnt, int64_t *__restrict__ tab_fix) {
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= K) return;
    const int64_t sa = slot_a[k], sb = slot_b[k];
    const uint64_t *__restrict__ ra = bits + sa * 5 * W, *__restrict__ rb = bits + sb * 5 * W;
    const uint32_t pa = seen[sa], pb = seen[sb];
    LinTable tot, t;
    lin_zero(tot);
    for (int32_t j = 0; j < n_jobs; ++j) {
        const int32_t first = job_first[j], count = job_count[j];
        int32_t mine = -1;   // the cluster whose table this lane holds after the job
        lin_zero(t);
        if (count == 0) {
            lin_walk(t, ra, rb, W, pa, pb, pc_word, pc_mask, pc_v, clu_piece[first], clu_piece[first + 1], lane, 64);
            lin_add(tot, t);
            lin_reduce(t, pa, pb);
            if (lane == 0) mine = first;
        } else if (lane < count) {
            mine = small[first + lane];
            lin_walk(t, ra, rb, W, pa, pb, pc_word, pc_mask, pc_v, clu_piece[mine], clu_piece[mine + 1], 0, 1);
            lin_add(tot, t);
        }
        if (mine >= 0) {
            uint32_t pl = 0;
            const double v = lin_eval(t, scale, neff[mine], &pl);
            const int64_t o = k * C + mine;
            mi[o] = v;
            poly[o] = (uint8_t)pl;
            if (tab_cnt) {
#pragma unroll
                for (int q = 0; q < 25; ++q) tab_cnt[o * 25 + q] = t.cnt[q], tab_fix[o * 25 + q] = t.fix[q];
            }
        }
    }
    lin_reduce(tot, pa, pb);
    if (lane == 0) {
        uint32_t pl = 0;
        mi_all[k] = lin_eval(tot, scale, neff[C], &pl);
    }
}

}  // namespace ldw

namespace {

struct CluBufs {   // the working memory of one ldw_seq_clusters call
    ldw::HamBufs ham;
    ldw::DevBuf adj, f, changed, root, rank, label, scan;
};

int clusters_run(ldw_ctx *c, const int32_t *thresh, int32_t n_thresh, int32_t *labels_out, int32_t *n_out, CluBufs &b) {
    const char *who = "ldw_seq_clusters";
    LDW_REQUIRE(ldw::have_alignment(c), LDW_ERR_STATE, "%s: no alignment resident: set the alignment first", who);
    LDW_REQUIRE(thresh && labels_out && n_out, LDW_ERR_ARG, "%s: thresh, labels_out or n_clusters_out is null", who);
    LDW_REQUIRE(n_thresh >= 1 && n_thresh <= CLU_MAX_THRESH, LDW_ERR_ARG, "%s: %d thresholds (1..%d)", who, (int)n_thresh, CLU_MAX_THRESH);
    for (int32_t g = 0; g < n_thresh; ++g) LDW_REQUIRE(thresh[g] >= 0, LDW_ERR_ARG, "%s: thresh[%d] = %d is negative", who, (int)g, (int)thresh[g]);
    const int64_t N = c->N, L = c->L, KW = c->KW;
    LDW_REQUIRE(N < (1ll << 31) - 1, LDW_ERR_ARG, "%s: too many sequences", who);
    const int per_read = (int)std::max<int64_t>(1, std::min<int64_t>(n_thresh, CLU_ADJ_BYTES / (N * KW * 8)));
    int rc = LDW_OK;
    size_t scan_bytes = 0;
    LDW_HIP(ldw::prim_scan_bytes<int32_t>((size_t)N + 1, c->stream, &scan_bytes));
    if ((rc = b.adj.reserve((size_t)per_read * N * KW * 8)) || (rc = b.f.reserve((size_t)per_read * N * 4)) || (rc = b.changed.reserve(4)) ||
        (rc = b.root.reserve((size_t)(N + 1) * 4)) || (rc = b.rank.reserve((size_t)(N + 1) * 4)) || (rc = b.label.reserve((size_t)N * 4)) ||
        (rc = b.scan.reserve(scan_bytes + 256)))
        return rc;
    ldw::HamClock clk;
    if ((rc = ldw::hamming_gram(c, b.ham, -1, -1, clk, nullptr))) return rc;   // (records ev[0] first)
    const unsigned rows4 = (unsigned)ceil_div(N, 4), rows256 = (unsigned)ceil_div(N, 256);
    int32_t *f = b.f.as<int32_t>();
    uint32_t *changed = b.changed.as<uint32_t>();
    ldw::Laps laps;   // a pair of events per read of G, around its rounds
    int rounds_max = 0;
    for (int g0 = 0; g0 < n_thresh; g0 += per_read) {
        const int ng = std::min<int>(per_read, n_thresh - g0);
        ldw::CluThresh th{};
        th.n = ng;
        for (int g = 0; g < ng; ++g) th.t[g] = thresh[g0 + g];
        hipLaunchKernelGGL(k_clu_adj, dim3(rows4, (unsigned)KW), dim3(256), 0, c->stream, b.ham.Gh.as<int64_t>(), (int)c->Npad, b.ham.scnt.as<int32_t>(), N, L, KW, th,
                           b.adj.as<uint64_t>());
        hipLaunchKernelGGL(k_clu_init, dim3(rows256), dim3(256), 0, c->stream, N, ng, f);
        LDW_HIP(hipGetLastError());
        if (g0 + ng == n_thresh) {   // G (Npad^2 x 8 bytes) goes before the rounds of the last read
            LDW_HIP(hipStreamSynchronize(c->stream));
            ldw::DrainedScope quiet;
            b.ham = ldw::HamBufs();
        }
        if ((rc = laps.mark(c->stream))) return rc;
        uint32_t active = ng == 32 ? 0xFFFFFFFFu : ((1u << ng) - 1u);
        for (int round = 1; active; ++round) {
            LDW_HIP(hipMemsetAsync(changed, 0, 4, c->stream));
            hipLaunchKernelGGL(k_clu_hook, dim3(rows4, (unsigned)ng), dim3(256), 0, c->stream, b.adj.as<uint64_t>(), N, KW, active, f, changed);
            hipLaunchKernelGGL(k_clu_jump, dim3(rows256, (unsigned)ng), dim3(256), 0, c->stream, N, active, f, changed);
            LDW_HIP(hipGetLastError());
            uint32_t moved = 0;
            LDW_HIP(hipMemcpyAsync(&moved, changed, 4, hipMemcpyDeviceToHost, c->stream));
            LDW_HIP(hipStreamSynchronize(c->stream));
            active &= moved;
            rounds_max = std::max(rounds_max, round);
            LDW_REQUIRE(round <= N + 1, LDW_ERR_HIP, "%s: internal: the rounds do not end", who);
        }
        if ((rc = laps.mark(c->stream))) return rc;
        for (int g = 0; g < ng; ++g) {
            const int32_t *fg = f + (int64_t)g * N;
            hipLaunchKernelGGL(k_clu_roots, dim3((unsigned)ceil_div(N + 1, 256)), dim3(256), 0, c->stream, N, fg, b.root.as<int32_t>());
            LDW_HIP(hipGetLastError());
            LDW_HIP(ldw::prim_exclusive_sum<int32_t>(b.scan.p, scan_bytes, b.root.as<int32_t>(), b.rank.as<int32_t>(), (size_t)N + 1, c->stream));
            hipLaunchKernelGGL(k_clu_labels, dim3(rows256), dim3(256), 0, c->stream, N, fg, b.rank.as<int32_t>(), b.label.as<int32_t>());
            LDW_HIP(hipGetLastError());
            LDW_HIP(hipMemcpyAsync(labels_out + (int64_t)(g0 + g) * N, b.label.p, (size_t)N * 4, hipMemcpyDeviceToHost, c->stream));
            LDW_HIP(hipMemcpyAsync(n_out + g0 + g, b.rank.as<int32_t>() + N, 4, hipMemcpyDeviceToHost, c->stream));
            LDW_HIP(hipStreamSynchronize(c->stream));   // (label and rank are written again for the next threshold)
        }
    }
    // the rounds' time: between each read's pair of events; what ran in front: ev[0] (hamming_gram's) to the first event, and between the reads
    double t_rounds = 0;
    float t_total = 0;
    if ((rc = laps.sums(1, &t_rounds, 2))) return rc;
    LDW_HIP(hipEventElapsedTime(&t_total, c->ev[0], laps.ev.back()));
    c->last_ms[0] = t_rounds;
    c->last_ms[1] = (double)t_total - t_rounds;   // the Hamming GEMM, the adjacency bits (and, between two reads of G, the labels of the first)
    c->last_ms[2] = (double)rounds_max;           // rounds of the threshold that took most
    c->last_ms[3] = t_total;
    return LDW_OK;
}

struct LinBufs {   // the working memory of one ldw_links_stratified call
    ldw::DevBuf perm, pc_word, pc_mask, pc_v, clu_piece, job_first, job_count, small, neff, snp, slot_a, slot_b, bits, seen, mi, poly, mi_all, tab_cnt, tab_fix;
};

int stratified_run(ldw_ctx *c, const int32_t *pair_a, const int32_t *pair_b, int64_t K, const int32_t *labels, int32_t C, double *mi_out, double *mi_all_out,
                   uint8_t *poly_out, double *neff_out, int64_t *counts_out, int64_t *fixed_out, int *frac_bits_out, LinBufs &b) {
    const char *who = "ldw_links_stratified";
    LDW_REQUIRE(ldw::have_alignment(c), LDW_ERR_STATE, "%s: no alignment resident: set the alignment first", who);
    LDW_REQUIRE(c->wts.have_weights, LDW_ERR_STATE, "%s: no weights resident: set the weights first", who);
    LDW_REQUIRE(pair_a && pair_b && labels, LDW_ERR_ARG, "%s: pair_a, pair_b or labels is null", who);
    LDW_REQUIRE(mi_out && mi_all_out && poly_out && neff_out && frac_bits_out, LDW_ERR_ARG, "%s: a required output is null", who);
    LDW_REQUIRE((counts_out == nullptr) == (fixed_out == nullptr), LDW_ERR_ARG, "%s: counts_out and fixed_out go together", who);
    LDW_REQUIRE(K >= 1, LDW_ERR_ARG, "%s: %lld pairs (at least 1)", who, (long long)K);
    LDW_REQUIRE(K < (1ll << 31), LDW_ERR_ARG, "%s: too many pairs", who);
    LDW_REQUIRE(C >= 1 && C <= LIN_MAX_CLUSTERS, LDW_ERR_ARG, "%s: C = %d clusters (1..%d)", who, (int)C, LIN_MAX_CLUSTERS);
    const int64_t N = c->N, L = c->L;
    const ldw::LabelSet ls = ldw::LabelSet::scan(labels, N, C);
    LDW_REQUIRE(ls.bad < 0, LDW_ERR_ARG, "%s: labels[%lld] = %d (-1, or a cluster 0..%d)", who, (long long)ls.bad, (int)labels[ls.bad], (int)(C - 1));
    const int64_t P = ls.P;
    LDW_REQUIRE(P >= 1, LDW_ERR_ARG, "%s: every label is -1: no sequence to count", who);
    int64_t bad_k = -1;
    const int32_t *bad = ldw::first_bad_pair(pair_a, pair_b, K, L, &bad_k);
    LDW_REQUIRE(!bad, LDW_ERR_ARG, "%s: %s[%lld] = %d (the alignment has SNPs 0..%lld)", who, bad == pair_a ? "pair_a" : "pair_b", (long long)bad_k, (int)bad[bad_k], (long long)(L - 1));
    const std::vector<int64_t> &V = c->wts.h_vfixed;
    const std::vector<double> &hdw = c->wts.h_hdw;
    const bool want_tables = counts_out != nullptr;

    // ---- the order of the labelled sequences, the pieces, the clusters' ranges, the jobs (ldw_seq_plan.h) and the clusters' sums ----
    const ldw::LinPlan plan = ldw::build_lin_plan(labels, V.data(), N, C, P);
    const int64_t W = ceil_div(P, 64);
    const int32_t n_jobs = (int32_t)plan.job_first.size();
    std::vector<double> neff((size_t)C + 1);
    ldw::LabelSet::neff(labels, hdw.data(), N, C, neff.data());

    // ---- pairs per chunk: the rows of its distinct SNPs (2 k at most, and never more than L) and k rows of every output within the budget ----
    const int64_t row_bytes = 5 * W * 8 + 2 * 4, out_bytes = (int64_t)C * (8 + 1 + (want_tables ? 400 : 0)) + 8 + 2 * 4;
    int64_t chunk = L * row_bytes <= LIN_BUDGET / 2 ? (LIN_BUDGET - L * row_bytes) / out_bytes : LIN_BUDGET / (2 * row_bytes + out_bytes);
    chunk = ldw::budget_or_env(std::max<int64_t>(1, chunk), "LDW_LIN_CHUNK");
    chunk = std::min<int64_t>(std::min<int64_t>(chunk, K), (int64_t)1 << 24);
    int rc = LDW_OK;
    if ((rc = ldw::upload(c, b.perm, plan.perm.data(), plan.perm.size())) || (rc = ldw::upload(c, b.pc_word, plan.pc_word.data(), plan.pc_word.size())) ||
        (rc = ldw::upload(c, b.pc_mask, plan.pc_mask.data(), plan.pc_mask.size())) || (rc = ldw::upload(c, b.pc_v, plan.pc_v.data(), plan.pc_v.size())) ||
        (rc = ldw::upload(c, b.clu_piece, plan.clu_piece.data(), plan.clu_piece.size())) ||
        (rc = ldw::upload(c, b.job_first, plan.job_first.data(), plan.job_first.size())) ||
        (rc = ldw::upload(c, b.job_count, plan.job_count.data(), plan.job_count.size())) || (rc = ldw::upload(c, b.small, plan.small.data(), plan.small.size())) ||
        (rc = ldw::upload(c, b.neff, neff.data(), neff.size())))
        return rc;
    const size_t rows = (size_t)chunk * (size_t)C, d_max = (size_t)std::min<int64_t>(2 * chunk, L);
    if ((rc = b.snp.reserve(d_max * 4)) || (rc = b.slot_a.reserve((size_t)chunk * 4)) || (rc = b.slot_b.reserve((size_t)chunk * 4)) ||
        (rc = b.bits.reserve(d_max * 5 * (size_t)W * 8)) || (rc = b.seen.reserve(d_max * 4)) || (rc = b.mi.reserve(rows * 8)) ||
        (rc = b.poly.reserve(rows)) || (rc = b.mi_all.reserve((size_t)chunk * 8)) ||
        (want_tables && ((rc = b.tab_cnt.reserve(rows * 25 * 8)) || (rc = b.tab_fix.reserve(rows * 25 * 8)))))
        return rc;
    ldw::Laps laps;   // three events per chunk and one behind the last
    const double scale = std::ldexp(1.0, -c->wts.frac_bits);
    ldw::DistinctSlots ds;
    std::vector<int32_t> sa, sb;
    for (int64_t k0 = 0; k0 < K; k0 += chunk) {
        const int64_t k = std::min<int64_t>(chunk, K - k0);
        ds.assign(pair_a + k0, k, pair_b + k0, k);   // the distinct SNPs of the chunk
        sa.resize((size_t)k), sb.resize((size_t)k);
        for (int64_t i = 0; i < k; ++i) sa[(size_t)i] = ds.slot(pair_a[k0 + i]), sb[(size_t)i] = ds.slot(pair_b[k0 + i]);
        const int64_t D = (int64_t)ds.d.size();
        const size_t out_rows = (size_t)k * (size_t)C;
        if ((rc = laps.mark(c->stream))) return rc;
        LDW_HIP(hipMemcpyAsync(b.snp.p, ds.d.data(), (size_t)D * 4, hipMemcpyHostToDevice, c->stream));
        LDW_HIP(hipMemcpyAsync(b.slot_a.p, sa.data(), (size_t)k * 4, hipMemcpyHostToDevice, c->stream));
        LDW_HIP(hipMemcpyAsync(b.slot_b.p, sb.data(), (size_t)k * 4, hipMemcpyHostToDevice, c->stream));
        LDW_HIP(hipMemsetAsync(b.seen.p, 0, (size_t)D * 4, c->stream));
        hipLaunchKernelGGL(k_lin_bits, dim3((unsigned)D, (unsigned)ceil_div(W, 4)), dim3(256), 0, c->stream, c->states.as<uint8_t>(), c->Npad, b.snp.as<int32_t>(),
                           b.perm.as<int32_t>(), P, W, b.bits.as<uint64_t>(), b.seen.as<uint32_t>());
        LDW_HIP(hipGetLastError());
        if ((rc = laps.mark(c->stream))) return rc;
        LDW_HIP(hipMemsetAsync(b.mi.p, 0, out_rows * 8, c->stream));   // (a cluster without a member: 0 everywhere)
        LDW_HIP(hipMemsetAsync(b.poly.p, 0, out_rows, c->stream));
        if (want_tables) {
            LDW_HIP(hipMemsetAsync(b.tab_cnt.p, 0, out_rows * 25 * 8, c->stream));
            LDW_HIP(hipMemsetAsync(b.tab_fix.p, 0, out_rows * 25 * 8, c->stream));
        }
        hipLaunchKernelGGL(k_lin_pairs, dim3((unsigned)ceil_div(k, 4)), dim3(256), 0, c->stream, b.bits.as<uint64_t>(), b.seen.as<uint32_t>(), W, b.slot_a.as<int32_t>(),
                           b.slot_b.as<int32_t>(), k, C, b.job_first.as<int32_t>(), b.job_count.as<int32_t>(), n_jobs, b.small.as<int32_t>(), b.clu_piece.as<int64_t>(),
                           b.pc_word.as<int32_t>(), b.pc_mask.as<uint64_t>(), b.pc_v.as<int64_t>(), b.neff.as<double>(), scale, b.mi.as<double>(), b.poly.as<uint8_t>(),
                           b.mi_all.as<double>(), want_tables ? b.tab_cnt.as<int64_t>() : (int64_t *)nullptr, want_tables ? b.tab_fix.as<int64_t>() : (int64_t *)nullptr);
        LDW_HIP(hipGetLastError());
        if ((rc = laps.mark(c->stream))) return rc;
        LDW_HIP(hipMemcpyAsync(mi_out + k0 * C, b.mi.p, out_rows * 8, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipMemcpyAsync(poly_out + k0 * C, b.poly.p, out_rows, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipMemcpyAsync(mi_all_out + k0, b.mi_all.p, (size_t)k * 8, hipMemcpyDeviceToHost, c->stream));
        if (want_tables) {
            LDW_HIP(hipMemcpyAsync(counts_out + k0 * C * 25, b.tab_cnt.p, out_rows * 25 * 8, hipMemcpyDeviceToHost, c->stream));
            LDW_HIP(hipMemcpyAsync(fixed_out + k0 * C * 25, b.tab_fix.p, out_rows * 25 * 8, hipMemcpyDeviceToHost, c->stream));
        }
        LDW_HIP(hipStreamSynchronize(c->stream));   // (ds, sa and sb are filled again for the next chunk)
    }
    if ((rc = laps.mark(c->stream))) return rc;
    LDW_HIP(hipStreamSynchronize(c->stream));
    for (int32_t k = 0; k < C; ++k) neff_out[k] = neff[(size_t)k];
    *frac_bits_out = c->wts.frac_bits;
    double ms[3] = {0, 0, 0};
    if ((rc = laps.sums(3, ms))) return rc;
    c->last_ms[0] = ms[1];   // k_lin_pairs (with the zeroing of its outputs)
    c->last_ms[1] = ms[0];   // the chunk's uploads and k_lin_bits
    c->last_ms[2] = ms[2];   // the copies out
    c->last_ms[3] = ms[0] + ms[1] + ms[2];
    return LDW_OK;
}

}  // namespace

extern "C" int ldw_seq_clusters(ldw_ctx *c, const int32_t *thresh, int32_t n_thresh, int32_t *labels_out, int32_t *n_clusters_out) {
    return ldw::scoped_call<CluBufs>(c, [&](CluBufs &b) { return clusters_run(c, thresh, n_thresh, labels_out, n_clusters_out, b); });
}

extern "C" int ldw_links_stratified(ldw_ctx *c, const int32_t *pair_a, const int32_t *pair_b, int64_t K, const int32_t *labels, int32_t C, double *mi_out,
                                    double *mi_all_out, uint8_t *poly_out, double *neff_out, int64_t *counts_out, int64_t *fixed_out, int *frac_bits_out) {
    return ldw::scoped_call<LinBufs>(c, [&](LinBufs &b) {
        return stratified_run(c, pair_a, pair_b, K, labels, C, mi_out, mi_all_out, poly_out, neff_out, counts_out, fixed_out, frac_bits_out, b);
    });
}
