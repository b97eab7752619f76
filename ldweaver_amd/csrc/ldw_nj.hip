// Neighbour joining on the device: ldw_nj_tree builds the tree of the resident alignment's Hamming distances, d(i, j) = L - shared(i, j)
// from the Hamming stage's G and scnt, or of a caller's matrix; ldw_nj_bootstrap counts, per internal edge of that tree, the trees of resampled
// alignments that have the edge too (one more Hamming GEMM per replicate, the replicates' trees joined side by side, splits compared by sums of keys).
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
#include "ldw_seq_plan.h"

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

// The three kernels of a join and the root exist twice: for one tree (ldw_nj_tree) and for R trees side by side (ldw_nj_bootstrap: blockIdx.y is the
// tree, every pointer moved on by the tree's stride).  Both call the same body, so a tree's arithmetic and its order do not depend on which one ran.
__device__ __forceinline__ void nj_scan_body(const double *__restrict__ D, int64_t ld, const double *__restrict__ r, const int32_t *__restrict__ id, int32_t n,
                                             NjKey *__restrict__ part, NjKey *sh) {
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
__global__ __launch_bounds__(NJ_THREADS) void k_nj_scan(const double *__restrict__ D, int64_t ld, const double *__restrict__ r, const int32_t *__restrict__ id,
                                                        int32_t n, NjKey *__restrict__ part) {
    __shared__ NjKey sh[NJ_THREADS];
    nj_scan_body(D, ld, r, id, n, part, sh);
}

__device__ __forceinline__ void nj_finish_body(const double *__restrict__ D, int64_t ld, double *__restrict__ r, int32_t *__restrict__ id, int32_t n, int32_t u,
                                               const NjKey *__restrict__ part, int32_t n_part, NjJoin *__restrict__ join, int32_t *__restrict__ parent,
                                               double *__restrict__ length, NjKey *sh) {
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
__global__ __launch_bounds__(NJ_THREADS) void k_nj_finish(const double *__restrict__ D, int64_t ld, double *__restrict__ r, int32_t *__restrict__ id, int32_t n,
                                                          int32_t u, const NjKey *__restrict__ part, int32_t n_part, NjJoin *__restrict__ join,
                                                          int32_t *__restrict__ parent, double *__restrict__ length) {
    __shared__ NjKey sh[NJ_THREADS];
    nj_finish_body(D, ld, r, id, n, u, part, n_part, join, parent, length, sh);
}

// Thread k owns node k's entries: it reads D[sa][k], D[sb][k], D[last][k] and r[k] as they were before the join and writes row and column entries
// (su, k), (sd, k) only; nobody reads an entry another thread writes (d_ab comes from the join record, because the thread of the last slot writes
// d(u, last) where d_ab was).
__device__ __forceinline__ void nj_update_body(double *__restrict__ D, int64_t ld, double *__restrict__ r, int32_t *__restrict__ id, int32_t n,
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
__global__ __launch_bounds__(NJ_THREADS) void k_nj_update(double *__restrict__ D, int64_t ld, double *__restrict__ r, int32_t *__restrict__ id, int32_t n,
                                                          const NjJoin *__restrict__ join) {
    nj_update_body(D, ld, r, id, n, join);
}

// the three nodes left hang on the root; i < j < k by node id
__device__ __forceinline__ void nj_root_body(const double *__restrict__ D, int64_t ld, const int32_t *__restrict__ id, int32_t root, int32_t *__restrict__ parent,
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
__global__ void k_nj_root(const double *__restrict__ D, int64_t ld, const int32_t *__restrict__ id, int32_t root, int32_t *__restrict__ parent,
                          double *__restrict__ length) {
    nj_root_body(D, ld, id, root, parent, length);
}

// R trees side by side: tree t = blockIdx.y has its matrix at D + t sD, its r, id at + t sN, its partial keys at + t NJ_MAX_PARTIALS, its join record at
// + t, its parent and length at + t sP
struct NjBatch {
    int64_t sD, sN, sP;
};
__global__ __launch_bounds__(NJ_THREADS) void k_nj_scan_b(const double *__restrict__ D, int64_t ld, const double *__restrict__ r, const int32_t *__restrict__ id,
                                                          int32_t n, NjKey *__restrict__ part, NjBatch s) {
    __shared__ NjKey sh[NJ_THREADS];
    const int64_t t = blockIdx.y;
    nj_scan_body(D + t * s.sD, ld, r + t * s.sN, id + t * s.sN, n, part + t * NJ_MAX_PARTIALS, sh);
}
__global__ __launch_bounds__(NJ_THREADS) void k_nj_finish_b(const double *__restrict__ D, int64_t ld, double *__restrict__ r, int32_t *__restrict__ id, int32_t n,
                                                            int32_t u, const NjKey *__restrict__ part, int32_t n_part, NjJoin *__restrict__ join,
                                                            int32_t *__restrict__ parent, double *__restrict__ length, NjBatch s) {
    __shared__ NjKey sh[NJ_THREADS];
    const int64_t t = blockIdx.y;
    nj_finish_body(D + t * s.sD, ld, r + t * s.sN, id + t * s.sN, n, u, part + t * NJ_MAX_PARTIALS, n_part, join + t, parent + t * s.sP, length + t * s.sP, sh);
}
__global__ __launch_bounds__(NJ_THREADS) void k_nj_update_b(double *__restrict__ D, int64_t ld, double *__restrict__ r, int32_t *__restrict__ id, int32_t n,
                                                            const NjJoin *__restrict__ join, NjBatch s) {
    const int64_t t = blockIdx.y;
    nj_update_body(D + t * s.sD, ld, r + t * s.sN, id + t * s.sN, n, join + t);
}
__global__ void k_nj_root_b(const double *__restrict__ D, int64_t ld, const int32_t *__restrict__ id, int32_t root, int32_t *__restrict__ parent,
                            double *__restrict__ length, NjBatch s) {
    const int64_t t = blockIdx.y;
    nj_root_body(D + t * s.sD, ld, id + t * s.sN, root, parent + t * s.sP, length + t * s.sP);
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

// ---- bootstrap support -----------------------------------------------------------------------------------------------------------------

constexpr int NJ_MULT_CAP = 63;   // a biallelic column's digit is 2 and the GEMM's digit a signed int8: 2 x 63 = 126

// the Hamming GEMM's digit of column k under a replicate's multiplicities; zero in the padding
__global__ __launch_bounds__(NJ_THREADS) void k_boot_digits(const int8_t *__restrict__ dig, const int32_t *__restrict__ info, const int32_t *__restrict__ mult,
                                                            int64_t KR, int64_t Kpad, int8_t *__restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * NJ_THREADS + threadIdx.x;
    if (k >= Kpad) return;
    out[k] = k < KR ? (int8_t)((int32_t)dig[k] * mult[info[k] >> 4]) : (int8_t)0;
}

// row i of d_m(i, j) = (G_m(i, i) + G_m(j, j)) / 2 - G_m(i, j) from the lower-triangular G_m and its sum, as k_nj_fill
__global__ __launch_bounds__(NJ_THREADS) void k_boot_fill(const int64_t *__restrict__ G, int ldg, int64_t N, double *__restrict__ D, double *__restrict__ r,
                                                          int32_t *__restrict__ id) {
    __shared__ long long sh[NJ_THREADS];
    const int64_t i = blockIdx.x;
    const int64_t gii = G[i * ldg + i];
    long long sum = 0;
    for (int64_t j = threadIdx.x; j < N; j += NJ_THREADS) {
        const int64_t t = i < j ? i : j, f = i < j ? j : i;
        const int64_t d = i == j ? 0 : (gii + G[j * ldg + j]) / 2 - G[t * ldg + f];
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

// A split is named by a pair of 64-bit sums: tip t has the keys splitmix64(t + NJ_KEY1) and splitmix64(t + NJ_KEY2), a node the wrapping sums of the
// keys of the tips below it, and the split's canonical pair is the lexicographically smaller of (h1, h2) and (total1 - h1, total2 - h2): either side
// of the edge gives the same pair.
constexpr uint64_t NJ_KEY1 = 0x243F6A8885A308D3ull, NJ_KEY2 = 0x13198A2E03707344ull;
__host__ __device__ __forceinline__ uint64_t nj_splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
struct NjSplit {
    unsigned long long a, b;
};
__device__ __forceinline__ bool nj_split_less(const NjSplit &x, const NjSplit &y) { return (x.a < y.a) | ((x.a == y.a) & (x.b < y.b)); }
__device__ __forceinline__ bool nj_split_same(const NjSplit &x, const NjSplit &y) { return (x.a == y.a) & (x.b == y.b); }
__device__ __forceinline__ NjSplit nj_canon(unsigned long long h1, unsigned long long h2, unsigned long long t1, unsigned long long t2) {
    const NjSplit x{h1, h2}, y{t1 - h1, t2 - h2};
    const bool other = nj_split_less(y, x);
    return NjSplit{other ? y.a : x.a, other ? y.b : x.b};
}

// tree blockIdx.y (parent + y sP; its sums h + y 2 sP, zeroed: h1 of node v at [v], h2 at [sP + v]): every tip walks to the root and adds its keys to the
// join nodes on its way.  The walk ends at the root, at anything that is no join node, and after 2N steps whatever the array holds.
__global__ __launch_bounds__(NJ_THREADS) void k_boot_hash(const int32_t *__restrict__ parent, int64_t sP, int64_t N, unsigned long long *__restrict__ h) {
    const int64_t t = (int64_t)blockIdx.x * NJ_THREADS + threadIdx.x;
    if (t >= N) return;
    const int32_t *__restrict__ par = parent + (int64_t)blockIdx.y * sP;
    unsigned long long *__restrict__ hh = h + (int64_t)blockIdx.y * 2 * sP;
    const unsigned long long k1 = nj_splitmix64((uint64_t)t + NJ_KEY1), k2 = nj_splitmix64((uint64_t)t + NJ_KEY2);
    int64_t v = par[t];
    for (int64_t step = 0; step < 2 * N && v >= N && v < 2 * N - 3; ++step) {
        atomicAdd(&hh[v], k1);
        atomicAdd(&hh[sP + v], k2);
        v = par[v];
    }
}

// The reference tree's M = N - 3 canonical pairs in ascending order with their nodes.  Every pair finds its rank by counting the smaller ones (equal
// pairs by index): M^2 comparisons once per call, beside the M^3 / 3 entries the tree's own scans read.
__global__ __launch_bounds__(NJ_THREADS) void k_boot_ref_sort(const unsigned long long *__restrict__ h, int64_t sP, int64_t N, unsigned long long t1,
                                                              unsigned long long t2, NjSplit *__restrict__ sorted, int32_t *__restrict__ node) {
    const int64_t M = N - 3, i = (int64_t)blockIdx.x * NJ_THREADS + threadIdx.x;
    if (i >= M) return;
    const NjSplit mine = nj_canon(h[N + i], h[sP + N + i], t1, t2);
    int64_t rank = 0;
    for (int64_t j = 0; j < M; ++j) {
        const NjSplit x = nj_canon(h[N + j], h[sP + N + j], t1, t2);
        rank += (int)nj_split_less(x, mine) | ((int)nj_split_same(x, mine) & (int)(j < i));
    }
    sorted[rank] = mine;
    node[rank] = (int32_t)(N + i);
}

// join node N + i of tree blockIdx.y: its canonical pair, looked up among the reference's by binary search; a hit counts for that reference node
__global__ __launch_bounds__(NJ_THREADS) void k_boot_lookup(const unsigned long long *__restrict__ h, int64_t sP, int64_t N, unsigned long long t1,
                                                            unsigned long long t2, const NjSplit *__restrict__ sorted, const int32_t *__restrict__ node,
                                                            int32_t *__restrict__ support) {
    const int64_t M = N - 3, i = (int64_t)blockIdx.x * NJ_THREADS + threadIdx.x;
    if (i >= M) return;
    const unsigned long long *__restrict__ hh = h + (int64_t)blockIdx.y * 2 * sP;
    const NjSplit mine = nj_canon(hh[N + i], hh[sP + N + i], t1, t2);
    int64_t lo = 0, hi = M;   // the first entry that is not smaller
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const bool below = nj_split_less(sorted[mid], mine);
        lo = below ? mid + 1 : lo;
        hi = below ? hi : mid;
    }
    if (lo < M && nj_split_same(sorted[lo], mine)) atomicAdd(&support[node[lo]], 1);
}

// support of the join nodes N .. 2N-4 starts at 0; tips and the root have none: -1
__global__ __launch_bounds__(NJ_THREADS) void k_boot_support_init(int64_t N, int32_t *__restrict__ support) {
    const int64_t v = (int64_t)blockIdx.x * NJ_THREADS + threadIdx.x;
    if (v < 2 * N - 2) support[v] = (v >= N && v < 2 * N - 3) ? 0 : -1;
}

}  // namespace ldw

namespace {
struct NjBufs {   // the working memory of one call (nj_impl releases it)
    ldw::HamBufs ham;
    ldw::DevBuf D, r, id, part, join, parent, length, bad;
};
}  // namespace

// the N - 3 joins and the root of one tree whose d, r and id are in place, queued on the context's stream
static int nj_queue_tree(ldw_ctx *c, int64_t N, double *D, double *r, int32_t *id, NjKey *part, NjJoin *join, int32_t *parent, double *length) {
    for (int64_t s = 0; s + 3 < N; ++s) {
        const int32_t na = (int32_t)(N - s), u = (int32_t)(N + s), P = std::min<int32_t>(na, NJ_MAX_PARTIALS);
        hipLaunchKernelGGL(k_nj_scan, dim3((unsigned)P), dim3(NJ_THREADS), 0, c->stream, D, N, r, id, na, part);
        hipLaunchKernelGGL(k_nj_finish, dim3(1), dim3(NJ_THREADS), 0, c->stream, D, N, r, id, na, u, part, P, join, parent, length);
        hipLaunchKernelGGL(k_nj_update, dim3((unsigned)((na + NJ_THREADS - 1) / NJ_THREADS)), dim3(NJ_THREADS), 0, c->stream, D, N, r, id, na, join);
        if ((s & 255) == 255) LDW_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_nj_root, dim3(1), dim3(64), 0, c->stream, D, N, id, (int32_t)(2 * N - 3), parent, length);
    LDW_HIP(hipGetLastError());
    return LDW_OK;
}

// the same for `trees` trees side by side (strides s): three launches per join for all of them
static int nj_queue_trees(ldw_ctx *c, int64_t N, int trees, const NjBatch &s, double *D, double *r, int32_t *id, NjKey *part, NjJoin *join, int32_t *parent,
                          double *length) {
    const unsigned T = (unsigned)trees;
    for (int64_t j = 0; j + 3 < N; ++j) {
        const int32_t na = (int32_t)(N - j), u = (int32_t)(N + j), P = std::min<int32_t>(na, NJ_MAX_PARTIALS);
        hipLaunchKernelGGL(k_nj_scan_b, dim3((unsigned)P, T), dim3(NJ_THREADS), 0, c->stream, D, N, r, id, na, part, s);
        hipLaunchKernelGGL(k_nj_finish_b, dim3(1, T), dim3(NJ_THREADS), 0, c->stream, D, N, r, id, na, u, part, P, join, parent, length, s);
        hipLaunchKernelGGL(k_nj_update_b, dim3((unsigned)((na + NJ_THREADS - 1) / NJ_THREADS), T), dim3(NJ_THREADS), 0, c->stream, D, N, r, id, na, join, s);
        if ((j & 255) == 255) LDW_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_nj_root_b, dim3(1, T), dim3(64), 0, c->stream, D, N, id, (int32_t)(2 * N - 3), parent, length, s);
    LDW_HIP(hipGetLastError());
    return LDW_OK;
}

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
    if ((rc = nj_queue_tree(c, N, D, r, id, part, join, parent, length))) return rc;
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
    return ldw::scoped_call<NjBufs>(c, [&](NjBufs &b) { return nj_run(c, dist, n, parent_out, length_out, b); });
}

// ---- bootstrap support ----------------------------------------------------------------------------------------------------------------------------------

constexpr int NJ_BATCH_CAP = 16;                      // most replicate trees joined side by side
constexpr int64_t NJ_BATCH_BYTES = (int64_t)4 << 30;   // their matrices together stay within this (more trees in flight still pay at 200 MB each)

namespace {
struct NjBootBufs {   // the working memory of one call: the single tree's, the replicate batch's (NjBufs tree holds T0's D in the batch's first matrix)
    NjBufs tree;
    ldw::DevBuf mult, digb, h, sorted, node, support;
};
}  // namespace

// the batch size R of this call: LDW_NJ_BATCH=k forces k (a test hook, read at every call); never more than B
static int64_t nj_batch_size(int64_t B, int64_t N) {
    return std::min<int64_t>(ldw::budget_or_env(std::min<int64_t>(NJ_BATCH_CAP, std::max<int64_t>(1, NJ_BATCH_BYTES / (8 * N * N))), "LDW_NJ_BATCH"), B);
}

static int nj_boot_run(ldw_ctx *c, const int32_t *mult, int64_t B, int64_t n, int32_t *parent_out, double *length_out, int32_t *support_out,
                       int32_t *rep_parent_out, double *rep_length_out, NjBootBufs &b) {
    LDW_REQUIRE(ldw::have_alignment(c), LDW_ERR_STATE, "ldw_nj_bootstrap: no alignment resident: set the alignment first");
    LDW_REQUIRE(n == c->N, LDW_ERR_ARG, "ldw_nj_bootstrap: n = %lld but the resident alignment has %lld sequences", (long long)n, (long long)c->N);
    LDW_REQUIRE(n >= 3, LDW_ERR_ARG, "ldw_nj_bootstrap: %lld nodes (a tree needs at least 3)", (long long)n);
    LDW_REQUIRE(n < (1ll << 30), LDW_ERR_ARG, "ldw_nj_bootstrap: too many nodes");
    LDW_REQUIRE(B >= 1, LDW_ERR_ARG, "ldw_nj_bootstrap: %lld replicates (at least 1)", (long long)B);
    LDW_REQUIRE(B < (1ll << 30), LDW_ERR_ARG, "ldw_nj_bootstrap: too many replicates");
    LDW_REQUIRE(mult && parent_out && length_out && support_out, LDW_ERR_ARG, "ldw_nj_bootstrap: a required pointer is null");
    const int64_t N = n, L = c->L, sP = 2 * N - 2, M = N - 3;
    for (int64_t rep = 0; rep < B; ++rep) {
        int64_t sum = 0;
        for (int64_t a = 0; a < L; ++a) {
            const int32_t m = mult[rep * L + a];
            LDW_REQUIRE(m >= 0 && m <= NJ_MULT_CAP, LDW_ERR_ARG, "ldw_nj_bootstrap: replicate %lld has multiplicity %d at column %lld (0..%d)", (long long)rep,
                        (int)m, (long long)a, NJ_MULT_CAP);
            sum += m;
        }
        LDW_REQUIRE(sum < (1ll << 27), LDW_ERR_ARG, "ldw_nj_bootstrap: the multiplicities of replicate %lld add up to %lld (less than 2^27)", (long long)rep,
                    (long long)sum);
    }
    const int64_t R = nj_batch_size(B, N);
    const bool keep = rep_parent_out || rep_length_out;     // every replicate's tree stays on the device until the end
    const int64_t stored = keep ? B : R;
    NjBufs &t = b.tree;
    int rc = LDW_OK;
    if ((rc = t.D.reserve((size_t)R * N * N * 8)) || (rc = t.r.reserve((size_t)R * N * 8)) || (rc = t.id.reserve((size_t)R * N * 4)) ||
        (rc = t.part.reserve(sizeof(NjKey) * NJ_MAX_PARTIALS * (size_t)R)) || (rc = t.join.reserve(sizeof(NjJoin) * (size_t)R)) ||
        (rc = t.parent.reserve((size_t)(stored + 1) * sP * 4)) || (rc = t.length.reserve((size_t)(stored + 1) * sP * 8)) ||
        (rc = b.mult.reserve((size_t)R * L * 4)) || (rc = b.h.reserve((size_t)R * 2 * sP * 8)) || (rc = b.sorted.reserve(sizeof(NjSplit) * (size_t)std::max<int64_t>(M, 1))) ||
        (rc = b.node.reserve((size_t)std::max<int64_t>(M, 1) * 4)) || (rc = b.support.reserve((size_t)sP * 4)))
        return rc;
    double *D = t.D.as<double>(), *r = t.r.as<double>();
    int32_t *id = t.id.as<int32_t>();
    NjKey *part = t.part.as<NjKey>();
    NjJoin *join = t.join.as<NjJoin>();
    // tree 0 of parent / length is the reference tree T0, the replicates follow it
    int32_t *parent = t.parent.as<int32_t>(), *support = b.support.as<int32_t>(), *node = b.node.as<int32_t>();
    double *length = t.length.as<double>();
    unsigned long long *h = b.h.as<unsigned long long>();
    NjSplit *sorted = b.sorted.as<NjSplit>();
    uint64_t t1 = 0, t2 = 0;
    for (int64_t k = 0; k < N; ++k) t1 += nj_splitmix64((uint64_t)k + NJ_KEY1), t2 += nj_splitmix64((uint64_t)k + NJ_KEY2);
    const unsigned tip_grid = (unsigned)((N + NJ_THREADS - 1) / NJ_THREADS), join_grid = (unsigned)((std::max<int64_t>(M, 1) + NJ_THREADS - 1) / NJ_THREADS);

    // T0: the launches of ldw_nj_tree, except that G, T and the column records stay for the replicates
    ldw::HamClock clk;
    ldw::HamShape shape;
    if ((rc = ldw::hamming_gram(c, t.ham, -1, -1, clk, &shape))) return rc;
    const int ldg = (int)c->Npad;
    int64_t *G = t.ham.Gh.as<int64_t>();
    if ((rc = b.digb.reserve((size_t)shape.Kpad))) return rc;
    hipLaunchKernelGGL(k_nj_fill, dim3((unsigned)N), dim3(NJ_THREADS), 0, c->stream, G, ldg, t.ham.scnt.as<int32_t>(), N, L, D, r, id);
    LDW_HIP(hipGetLastError());
    if ((rc = nj_queue_tree(c, N, D, r, id, part, join, parent, length))) return rc;
    hipLaunchKernelGGL(k_boot_support_init, dim3((unsigned)((sP + NJ_THREADS - 1) / NJ_THREADS)), dim3(NJ_THREADS), 0, c->stream, N, support);
    if (M > 0) {
        LDW_HIP(hipMemsetAsync(h, 0, (size_t)2 * sP * 8, c->stream));
        hipLaunchKernelGGL(k_boot_hash, dim3(tip_grid, 1), dim3(NJ_THREADS), 0, c->stream, parent, sP, N, h);
        hipLaunchKernelGGL(k_boot_ref_sort, dim3(join_grid), dim3(NJ_THREADS), 0, c->stream, h, sP, N, (unsigned long long)t1, (unsigned long long)t2, sorted, node);
    }
    LDW_HIP(hipGetLastError());

    // the replicates, R at a time: digits, GEMM and fill one after the other into G (the stream orders them), then the joins of all R, their sums, the look-up
    const NjBatch strides{N * N, N, sP};
    const int64_t n_batches = (B + R - 1) / R;
    ldw::Laps laps;   // four events per batch: the three intervals between them count, what lies between two batches does not
    for (int64_t q = 0; q < n_batches; ++q) {
        const int64_t b0 = q * R, nb = std::min<int64_t>(R, B - b0);
        int32_t *bpar = parent + (1 + (keep ? b0 : 0)) * sP;
        double *blen = length + (1 + (keep ? b0 : 0)) * sP;
        if ((rc = laps.mark(c->stream))) return rc;
        LDW_HIP(hipMemcpyAsync(b.mult.p, mult + b0 * L, (size_t)nb * L * 4, hipMemcpyHostToDevice, c->stream));
        for (int64_t k = 0; k < nb; ++k) {
            hipLaunchKernelGGL(k_boot_digits, dim3((unsigned)((shape.Kpad + NJ_THREADS - 1) / NJ_THREADS)), dim3(NJ_THREADS), 0, c->stream, t.ham.dig.as<int8_t>(),
                               t.ham.info.as<int32_t>(), b.mult.as<int32_t>() + k * L, shape.KR, shape.Kpad, b.digb.as<int8_t>());
            LDW_HIP(hipGetLastError());
            if ((rc = launch_gemm_bits(c, t.ham.T.as<uint64_t>(), shape.KWr, t.ham.rl.as<int32_t>(), ldg, t.ham.rl.as<int32_t>(), ldg, G, 1, b.digb.as<int8_t>(), 1)))
                return rc;
            hipLaunchKernelGGL(k_boot_fill, dim3((unsigned)N), dim3(NJ_THREADS), 0, c->stream, G, ldg, N, D + k * N * N, r + k * N, id + k * N);
            LDW_HIP(hipGetLastError());
        }
        if ((rc = laps.mark(c->stream))) return rc;
        // (a batch of one takes the single tree's kernels: the same bodies, and 6.2 ms instead of 7.8 for a launch-bound tree of 616 tips)
        if ((rc = nb == 1 ? nj_queue_tree(c, N, D, r, id, part, join, bpar, blen) : nj_queue_trees(c, N, (int)nb, strides, D, r, id, part, join, bpar, blen)))
            return rc;
        if ((rc = laps.mark(c->stream))) return rc;
        if (M > 0) {
            LDW_HIP(hipMemsetAsync(h, 0, (size_t)nb * 2 * sP * 8, c->stream));
            hipLaunchKernelGGL(k_boot_hash, dim3(tip_grid, (unsigned)nb), dim3(NJ_THREADS), 0, c->stream, bpar, sP, N, h);
            hipLaunchKernelGGL(k_boot_lookup, dim3(join_grid, (unsigned)nb), dim3(NJ_THREADS), 0, c->stream, h, sP, N, (unsigned long long)t1, (unsigned long long)t2,
                               sorted, node, support);
            LDW_HIP(hipGetLastError());
        }
        if ((rc = laps.mark(c->stream))) return rc;
    }
    LDW_HIP(hipMemcpyAsync(parent_out, parent, (size_t)sP * 4, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemcpyAsync(length_out, length, (size_t)sP * 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemcpyAsync(support_out, support, (size_t)sP * 4, hipMemcpyDeviceToHost, c->stream));
    if (rep_parent_out) LDW_HIP(hipMemcpyAsync(rep_parent_out, parent + sP, (size_t)B * sP * 4, hipMemcpyDeviceToHost, c->stream));
    if (rep_length_out) LDW_HIP(hipMemcpyAsync(rep_length_out, length + sP, (size_t)B * sP * 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    double ms[3] = {0, 0, 0};
    if ((rc = laps.sums(3, ms, 4))) return rc;
    c->last_ms[0] = ms[1];                     // the replicates' joins and roots
    c->last_ms[1] = ms[0];                     // their multiplicities, digits, GEMMs and fills
    c->last_ms[2] = ms[2];                     // their sums and look-ups
    c->last_ms[3] = ms[0] + ms[1] + ms[2];
    return LDW_OK;
}

extern "C" int ldw_nj_bootstrap(ldw_ctx *c, const int32_t *mult, int64_t B, int64_t n, int32_t *parent_out, double *length_out, int32_t *support_out,
                                int32_t *rep_parent_out, double *rep_length_out) {
    return ldw::scoped_call<NjBootBufs>(
        c, [&](NjBootBufs &b) { return nj_boot_run(c, mult, B, n, parent_out, length_out, support_out, rep_parent_out, rep_length_out, b); });
}
