// Neighbour joining on the device: ldw_nj_tree builds the tree of the resident alignment's Hamming distances, d(i, j) = L - shared(i, j)
// from the Hamming stage's G and scnt, or of a caller's matrix.
//
// The active nodes live in SLOTS 0 .. n-1: the distance matrix is the top-left n x n of D (fp64, leading dimension N, both triangles kept), r[slot]
// the row sum, id[slot] the node.  Join s (n = N - s active nodes) is three launches, ordered by the stream alone:
//   k_nj_scan    Q over the n x n slots; workgroup w takes rows w, w + P, ... (P = min(n, NJ_MAX_PARTIALS)) and leaves its smallest key in part[w];
//   k_nj_finish  one workgroup: the smallest of the P keys, the branch lengths, r_u, parent and length of a and b, the join record;
//   k_nj_update  one thread per slot k: d(u, k), r_k, and the move of the last slot into the freed one, all from the OLD rows of a, b and the last slot.
// A key is (Q, smaller node id, larger node id), compared in that order: the tie rule is on nodes, so the slot order is free.  u takes the slot of
// a — of b when a sits in the last slot — and the last slot moves into the other one, so that the n - 1 nodes left fill slots 0 .. n-2.
// Every formula is written as DESIGN.md states it and the file compiles without FMA contraction: the host restatement (tests/nj_ref.py) is
// bit-identical.
#pragma clang fp contract(off)
#include <algorithm>
#include <cmath>
#include <vector>

#include "ldw_internal.h"
#include "ldw_hamming.h"

using namespace ldw;

namespace ldw {

constexpr int NJ_THREADS = 256;        // threads of every workgroup here: the scan's column tile (tests/test_nj_gpu.py names both constants)
constexpr int NJ_MAX_PARTIALS = 512;   // workgroups of a scan = entries of part[]
constexpr int NJ_UNROLL = 4;           // column tiles a scan's workgroup takes per step

struct NjKey {   // the smallest Q a thread / workgroup has seen, with the pair's nodes and slots (lo < 0: none yet)
    double q;
    int32_t lo, hi, si, sj;
};
struct NjJoin {  // what k_nj_finish leaves for k_nj_update
    int32_t sa, sb;   // slots of a (the smaller node id) and b
    int32_t su, sd;   // the slot u takes; the slot the last one moves into (sd == n - 1: nothing moves)
    double dab;
};

// Branch-free on purpose: a key is taken by five selects under one predicate.  (Written with early returns and a struct assignment, hipcc 7.2 kept
// the old slots beside the new Q and ids whenever a thread's SECOND candidate won.)
__device__ __forceinline__ bool nj_less(double q, int32_t lo, int32_t hi, const NjKey &b) {
    return (b.lo < 0) | (q < b.q) | ((q == b.q) & ((lo < b.lo) | ((lo == b.lo) & (hi < b.hi))));
}
__device__ __forceinline__ void nj_keep(NjKey &best, double q, int32_t lo, int32_t hi, int32_t si, int32_t sj, bool valid = true) {
    const bool take = valid & nj_less(q, lo, hi, best);
    best.q = take ? q : best.q;
    best.lo = take ? lo : best.lo;
    best.hi = take ? hi : best.hi;
    best.si = take ? si : best.si;
    best.sj = take ? sj : best.sj;
}
__device__ __forceinline__ void nj_take(NjKey &best, const NjKey &x) {
    if (x.lo >= 0) nj_keep(best, x.q, x.lo, x.hi, x.si, x.sj);
}

// the smallest key of the workgroup, valid in thread 0
__device__ __forceinline__ NjKey nj_reduce(NjKey best, NjKey *sh) {
    const int tid = threadIdx.x;
    sh[tid] = best;
    __syncthreads();
#pragma unroll
    for (int off = NJ_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) {
            NjKey mine = sh[tid];
            nj_take(mine, sh[tid + off]);
            sh[tid] = mine;
        }
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(NJ_THREADS) void k_nj_scan(const double *__restrict__ D, int64_t ld, const double *__restrict__ r, const int32_t *__restrict__ id,
                                                        int32_t n, NjKey *__restrict__ part) {
    __shared__ NjKey sh[NJ_THREADS];
    const double nm2 = (double)(n - 2);
    NjKey best{0.0, -1, -1, -1, -1};
    for (int32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const double ri = r[i];
        const int32_t idi = id[i];
        const double *__restrict__ row = D + (int64_t)i * ld;
        // NJ_UNROLL column tiles per step, their loads issued before the first key is compared (one load in flight per thread left the scan
        // latency-bound); a column past n is loaded from column 0, and it and the diagonal are masked out
        for (int32_t j0 = threadIdx.x; j0 < n; j0 += NJ_UNROLL * NJ_THREADS) {
            double dv[NJ_UNROLL], rv[NJ_UNROLL];
            int32_t iv[NJ_UNROLL];
#pragma unroll
            for (int u = 0; u < NJ_UNROLL; ++u) {
                const int32_t j = j0 + u * NJ_THREADS, jj = j < n ? j : 0;
                dv[u] = row[jj], rv[u] = r[jj], iv[u] = id[jj];
            }
#pragma unroll
            for (int u = 0; u < NJ_UNROLL; ++u) {
                const int32_t j = j0 + u * NJ_THREADS;
                const double q = (nm2 * dv[u] - ri) - rv[u];
                const int32_t lo = idi < iv[u] ? idi : iv[u], hi = idi < iv[u] ? iv[u] : idi;
                nj_keep(best, q, lo, hi, i, j, (j < n) & (j != i));
            }
        }
    }
    best = nj_reduce(best, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = best;
}

__global__ __launch_bounds__(NJ_THREADS) void k_nj_finish(const double *__restrict__ D, int64_t ld, double *__restrict__ r, int32_t *__restrict__ id, int32_t n,
                                                          int32_t u, const NjKey *__restrict__ part, int32_t n_part, NjJoin *__restrict__ join,
                                                          int32_t *__restrict__ parent, double *__restrict__ length) {
    __shared__ NjKey sh[NJ_THREADS];
    NjKey best{0.0, -1, -1, -1, -1};
    for (int32_t p = threadIdx.x; p < n_part; p += NJ_THREADS) nj_take(best, part[p]);
    best = nj_reduce(best, sh);
    if (threadIdx.x != 0) return;
    const int32_t sa = id[best.si] == best.lo ? best.si : best.sj, sb = sa == best.si ? best.sj : best.si;
    const double dab = D[(int64_t)sa * ld + sb], ra = r[sa], rb = r[sb];
    const double la = 0.5 * dab + (ra - rb) / (2.0 * (double)(n - 2));
    const double lb = dab - la;
    const double ru = ((ra + rb) - (double)n * dab) * 0.5;
    parent[best.lo] = u, parent[best.hi] = u;
    length[best.lo] = la, length[best.hi] = lb;
    const int32_t su = sa == n - 1 ? sb : sa, sd = sa == n - 1 ? sa : sb;
    r[su] = ru;
    id[su] = u;
    *join = NjJoin{sa, sb, su, sd, dab};
}

// Thread k owns node k's entries: it reads D[sa][k], D[sb][k], D[last][k] and r[k] as they were before the join and writes row and column entries
// (su, k), (sd, k) only; nobody reads an entry another thread writes (d_ab comes from the join record, because the thread of the last slot writes
// d(u, last) where d_ab was).
__global__ __launch_bounds__(NJ_THREADS) void k_nj_update(double *__restrict__ D, int64_t ld, double *__restrict__ r, int32_t *__restrict__ id, int32_t n,
                                                          const NjJoin *__restrict__ join) {
    const int32_t k = (int32_t)(blockIdx.x * NJ_THREADS + threadIdx.x);
    const NjJoin J = *join;
    if (k >= n || k == J.su || k == J.sd) return;
    const int32_t last = n - 1;
    const double dak = D[(int64_t)J.sa * ld + k], dbk = D[(int64_t)J.sb * ld + k];
    const double duk = ((dak + dbk) - J.dab) * 0.5;
    const double rk = ((r[k] - dak) - dbk) + duk;
    const int32_t dst = k == last ? J.sd : k;   // where node k lives after the join
    if (k != last && J.sd != last) {
        const double m = D[(int64_t)last * ld + k];
        D[(int64_t)J.sd * ld + k] = m;
        D[(int64_t)k * ld + J.sd] = m;
    }
    D[(int64_t)J.su * ld + dst] = duk;
    D[(int64_t)dst * ld + J.su] = duk;
    r[dst] = rk;
    if (k == last) id[J.sd] = id[last];
}

// the three nodes left hang on the root; i < j < k by node id
__global__ void k_nj_root(const double *__restrict__ D, int64_t ld, const int32_t *__restrict__ id, int32_t root, int32_t *__restrict__ parent,
                          double *__restrict__ length) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int32_t s[3] = {0, 1, 2};
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2 - a; ++b)
            if (id[s[b]] > id[s[b + 1]]) {
                const int32_t t = s[b];
                s[b] = s[b + 1], s[b + 1] = t;
            }
    const double dij = D[(int64_t)s[0] * ld + s[1]], dik = D[(int64_t)s[0] * ld + s[2]], djk = D[(int64_t)s[1] * ld + s[2]];
    length[id[s[0]]] = ((dij + dik) - djk) * 0.5;
    length[id[s[1]]] = ((djk + dij) - dik) * 0.5;
    length[id[s[2]]] = ((dik + djk) - dij) * 0.5;
    for (int a = 0; a < 3; ++a) parent[id[s[a]]] = root;
    parent[root] = -1;
    length[root] = 0.0;
}

// ---- initialisation ---------------------------------------------------------------------------------------------------------------------------------

// row i of d = L - shared and its sum: one workgroup per row; the entries are integers, so is the sum (int64: exact in any order)
__global__ __launch_bounds__(NJ_THREADS) void k_nj_fill(const int64_t *__restrict__ G, int ldg, const int32_t *__restrict__ cnt, int64_t N, int64_t L,
                                                        double *__restrict__ D, double *__restrict__ r, int32_t *__restrict__ id) {
    __shared__ long long sh[NJ_THREADS];
    const int64_t i = blockIdx.x;
    long long sum = 0;
    for (int64_t j = threadIdx.x; j < N; j += NJ_THREADS) {
        const int64_t d = i == j ? 0 : L - shared_ij(G, ldg, cnt, L, i, j);
        D[i * N + j] = (double)d;
        sum += d;
    }
    sh[threadIdx.x] = sum;
    __syncthreads();
    for (int off = NJ_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) r[i] = (double)sh[0], id[i] = (int32_t)i;
}

// a caller's matrix: bad[0] |= 1 not finite, 2 not bitwise symmetric, 4 diagonal not zero
__global__ __launch_bounds__(NJ_THREADS) void k_nj_check(const double *__restrict__ D, int64_t N, uint32_t *__restrict__ bad) {
    const int64_t t = (int64_t)blockIdx.x * NJ_THREADS + threadIdx.x;
    if (t >= N * N) return;
    const int64_t i = t / N, j = t - i * N;
    const double x = D[t];
    uint32_t f = 0;
    if (!(fabs(x) <= 1.7976931348623157e308)) f |= 1u;
    if (__double_as_longlong(x) != __double_as_longlong(D[j * N + i])) f |= 2u;
    if (i == j && x != 0.0) f |= 4u;
    if (f) atomicOr(bad, f);
}

// r_i = the sum of d(k, i) over k = 0, 1, ..., N-1 in that order, one thread per i (column reads of the symmetric matrix coalesce)
__global__ __launch_bounds__(NJ_THREADS) void k_nj_rowsum(const double *__restrict__ D, int64_t N, double *__restrict__ r, int32_t *__restrict__ id) {
    const int64_t i = (int64_t)blockIdx.x * NJ_THREADS + threadIdx.x;
    if (i >= N) return;
    double s = 0.0;
    for (int64_t k = 0; k < N; ++k) s = s + D[k * N + i];
    r[i] = s;
    id[i] = (int32_t)i;
}

}  // namespace ldw

namespace {
struct NjBufs {   // the working memory of one call (nj_impl releases it)
    ldw::HamBufs ham;
    ldw::DevBuf D, r, id, part, join, parent, length, bad;
};
}  // namespace

static int nj_run(ldw_ctx *c, const double *dist, int64_t n, int32_t *parent_out, double *length_out, NjBufs &b) {
    LDW_REQUIRE(parent_out && length_out, LDW_ERR_ARG, "ldw_nj_tree: output is null");
    if (!dist) {
        LDW_REQUIRE(ldw::have_alignment(c), LDW_ERR_STATE, "ldw_nj_tree: no matrix given and no alignment resident: set the alignment first");
        LDW_REQUIRE(n == c->N, LDW_ERR_ARG, "ldw_nj_tree: n = %lld but the resident alignment has %lld sequences", (long long)n, (long long)c->N);
    }
    LDW_REQUIRE(n >= 3, LDW_ERR_ARG, "ldw_nj_tree: %lld nodes (a tree needs at least 3)", (long long)n);
    LDW_REQUIRE(n < (1ll << 30), LDW_ERR_ARG, "ldw_nj_tree: too many nodes");
    const int64_t N = n;
    int rc = LDW_OK;
    if ((rc = b.D.reserve((size_t)N * N * 8)) || (rc = b.r.reserve((size_t)N * 8)) || (rc = b.id.reserve((size_t)N * 4)) ||
        (rc = b.part.reserve(sizeof(NjKey) * NJ_MAX_PARTIALS)) || (rc = b.join.reserve(sizeof(NjJoin))) || (rc = b.parent.reserve((size_t)(2 * N - 2) * 4)) ||
        (rc = b.length.reserve((size_t)(2 * N - 2) * 8)) || (rc = b.bad.reserve(4)))
        return rc;
    double *D = b.D.as<double>(), *r = b.r.as<double>();
    int32_t *id = b.id.as<int32_t>();
    const unsigned row_grid = (unsigned)((N + NJ_THREADS - 1) / NJ_THREADS);
    if (dist) {
        LDW_HIP(hipEventRecord(c->ev[0], c->stream));
        LDW_HIP(hipMemcpyAsync(D, dist, (size_t)N * N * 8, hipMemcpyHostToDevice, c->stream));
        LDW_HIP(hipMemsetAsync(b.bad.p, 0, 4, c->stream));
        LDW_REQUIRE(N * N < ((int64_t)1 << 39), LDW_ERR_SIZE, "ldw_nj_tree: %lld x %lld entries exceed the launch grid", (long long)N, (long long)N);
        hipLaunchKernelGGL(k_nj_check, dim3((unsigned)((N * N + NJ_THREADS - 1) / NJ_THREADS)), dim3(NJ_THREADS), 0, c->stream, D, N, b.bad.as<uint32_t>());
        LDW_HIP(hipGetLastError());
        uint32_t bad = 0;
        LDW_HIP(hipMemcpyAsync(&bad, b.bad.p, 4, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipStreamSynchronize(c->stream));
        LDW_REQUIRE(!bad, LDW_ERR_ARG, "ldw_nj_tree: the matrix%s%s%s", bad & 1 ? " has an entry that is not finite;" : "",
                    bad & 2 ? " is not symmetric bit for bit;" : "", bad & 4 ? " has a diagonal entry that is not zero;" : "");
        hipLaunchKernelGGL(k_nj_rowsum, dim3(row_grid), dim3(NJ_THREADS), 0, c->stream, D, N, r, id);
        LDW_HIP(hipGetLastError());
    } else {
        ldw::HamClock clk;
        if ((rc = ldw::hamming_gram(c, b.ham, -1, -1, clk, nullptr))) return rc;   // (records ev[0] first)
        hipLaunchKernelGGL(k_nj_fill, dim3((unsigned)N), dim3(NJ_THREADS), 0, c->stream, b.ham.Gh.as<int64_t>(), (int)c->Npad, b.ham.scnt.as<int32_t>(), N, c->L,
                           D, r, id);
        LDW_HIP(hipGetLastError());
        // G (Npad^2 x 8 bytes) goes before the joins: nothing else of this call waits for the device until they are all queued
        LDW_HIP(hipStreamSynchronize(c->stream));
        ldw::DrainedScope quiet;
        b.ham = ldw::HamBufs();
    }
    LDW_HIP(hipEventRecord(c->ev[1], c->stream));
    int32_t *parent = b.parent.as<int32_t>();
    double *length = b.length.as<double>();
    NjKey *part = b.part.as<NjKey>();
    NjJoin *join = b.join.as<NjJoin>();
    for (int64_t s = 0; s + 3 < N; ++s) {
        const int32_t na = (int32_t)(N - s), u = (int32_t)(N + s), P = std::min<int32_t>(na, NJ_MAX_PARTIALS);
        hipLaunchKernelGGL(k_nj_scan, dim3((unsigned)P), dim3(NJ_THREADS), 0, c->stream, D, N, r, id, na, part);
        hipLaunchKernelGGL(k_nj_finish, dim3(1), dim3(NJ_THREADS), 0, c->stream, D, N, r, id, na, u, part, P, join, parent, length);
        hipLaunchKernelGGL(k_nj_update, dim3((unsigned)((na + NJ_THREADS - 1) / NJ_THREADS)), dim3(NJ_THREADS), 0, c->stream, D, N, r, id, na, join);
        if ((s & 255) == 255) LDW_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_nj_root, dim3(1), dim3(64), 0, c->stream, D, N, id, (int32_t)(2 * N - 3), parent, length);
    LDW_HIP(hipGetLastError());
    LDW_HIP(hipEventRecord(c->ev[3], c->stream));
    LDW_HIP(hipMemcpyAsync(parent_out, parent, (size_t)(2 * N - 2) * 4, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemcpyAsync(length_out, length, (size_t)(2 * N - 2) * 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    float t_init = 0, t_join = 0;
    LDW_HIP(hipEventElapsedTime(&t_init, c->ev[0], c->ev[1]));
    LDW_HIP(hipEventElapsedTime(&t_join, c->ev[1], c->ev[3]));
    c->last_ms[0] = t_join;                    // the joins and the root
    c->last_ms[1] = t_init;                    // upload + check + row sums, or the Hamming GEMM + the fill
    c->last_ms[2] = 3.0;                       // launches per join
    c->last_ms[3] = (double)t_init + t_join;
    return LDW_OK;
}

extern "C" int ldw_nj_tree(ldw_ctx *c, const double *dist, int64_t n, int32_t *parent_out, double *length_out) {
    if (int rc = check_gpu(c)) return rc;
    NjBufs bufs;
    const int rc = nj_run(c, dist, n, parent_out, length_out, bufs);
    // as hamming_impl: this context's stream alone touched the blocks
    if (hipStreamSynchronize(c->stream) == hipSuccess) {
        ldw::DrainedScope quiet;
        bufs = NjBufs();
    }
    return rc;
}
