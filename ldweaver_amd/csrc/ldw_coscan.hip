// The co-change scan (ldweaver_amd.h 23): over EVERY pair of the SNPs that change on at least min_changes branches of a tree, the number of
// branches on which both change, co = popcount(bits_i & bits_j), from the bitmaps k_pars_down leaves (ldw_pars.hip).  ldw_tree_cochange_scan gives the
// histogram of co over the qualifying pairs and, per SNP, its largest co and its partners at or above min_co; ldw_tree_cochange_links lists the pairs and
// names each SNP's best partner.  Every output is an integer add, an integer maximum or an integer minimum.
//
// The bitmaps are word-major, bits[word][slot], so the two sides of a tile of CS_I x CS_J pairs come in differently:
//   the I side   a lane owns one slot and streams its own words: consecutive lanes read consecutive dwords;
//   the J side   is the same for every lane of the wave: the address of word w of row j0 + j is wave-uniform, so the CS_J words of a step arrive by scalar
//                loads and stay in scalar registers; nothing is staged in LDS;
//   the counts   a lane keeps one int32 per J row in registers: per pair and word one v_and_b32 with a scalar operand and one v_bcnt_u32_b32 that adds.
// The filters run once per pair behind the word loop: the i < j mask, the distance per pair (never a bound of the tile), the lift test in int64.
//   scan         co > 0 goes to a 1024-bin LDS histogram, co == 0 is counted in a register; a lane keeps the maximum and the count of its own slot; the J
//                rows combine through LDS (a maximum and one ballot-counted add per row and wave), then one global atomic per row and tile;
//   links        a ballot and ONE counter add per wave give the hits of a J row their places (k_score_links' way), the stores guarded by cap; the best
//                partner is a 32-bit minimum: lane-local for the I side, the first matching lane of a wave through LDS for a J row.
// The tile grid covers the tiles that hold a pair i < j, in bands of tile rows (a grid dimension holds 65 535; LDW_COSCAN_ROWS=k forces bands of k).
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "ldw_internal.h"
#include "ldw_dev.h"
#include "ldw_pars.h"
#include "ldw_seq_plan.h"

using namespace ldw;

namespace ldw {

constexpr int CS_I = 256;            // slots of a tile's I side: one per thread
constexpr int CS_J = 64;             // rows of its J side: one accumulator each
constexpr int CS_THREADS = CS_I;
constexpr int CS_BINS = 1024;        // hist_out: the qualifying pairs per min(co, 1023)
constexpr int CS_NSTAT = 3;          // [0] the pairs of P, [1] the qualifying pairs, [2] the pairs listed
constexpr int64_t CS_MAX_NODES = (int64_t)1 << 21;
constexpr int64_t CS_MAX_LIFT = (int64_t)1 << 20;
constexpr int64_t CS_MAX_BAND = 65535;   // tile rows of a launch
static_assert(CS_I % CS_J == 0 && CS_J == 64, "a band's first tile column is a whole number of J tiles; a J row is a bit of a ballot");

struct CoArgs {
    const uint32_t *bits;            // [words][stride]: word w of slot s at bits[w stride + s]; the slots M .. stride - 1 are zero
    int64_t stride, words, M;
    const int32_t *changes, *idx, *pos;   // [stride] per slot: the score, the global SNP, the position (null without a distance)
    double g, min_len;               // min_len < 0: no distance
    int64_t B, min_lift;
    int32_t min_co;
    int64_t ti0, tj0;                // the first tile row and the first tile column of this launch
    unsigned long long *hist;        // scan: [CS_BINS]
    int32_t *best;                   // scan: [M], -1 = none
    unsigned long long *nge;         // scan: [M]
    const int32_t *best_in;          // links: [stride] (null: no partners wanted)
    int32_t *partner;                // links: [M], INT_MAX = none
    unsigned long long cap;
    int32_t *la, *lb, *lco;
    unsigned long long *stat;        // [CS_NSTAT]
};

template <bool LINKS> __global__ __launch_bounds__(CS_THREADS) void k_coscan(CoArgs A) {
    __shared__ uint32_t s_hist[LINKS ? 1 : CS_BINS];
    __shared__ int32_t s_row[CS_J];      // scan: the largest co of a J row; links: its smallest matching partner
    __shared__ uint32_t s_nge[CS_J];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t i0 = (A.ti0 + (int64_t)blockIdx.y) * CS_I, j0 = (A.tj0 + (int64_t)blockIdx.x) * CS_J;
    if (j0 + CS_J - 1 <= i0) return;   // no pair a < b in the tile
    if (!LINKS)
        for (int i = tid; i < CS_BINS; i += CS_THREADS) s_hist[i] = 0;
    if (tid < CS_J) s_row[tid] = LINKS ? INT_MAX : -1, s_nge[tid] = 0;
    __syncthreads();

    const int64_t a = i0 + tid;          // (a < stride: the stride is a multiple of CS_I)
    int32_t acc[CS_J];
#pragma unroll
    for (int j = 0; j < CS_J; ++j) acc[j] = 0;
    const uint32_t *__restrict__ mine = A.bits + a, *__restrict__ rows = A.bits + j0;
    // (no vectoriser: it versions the loop for a stride of 1, two words at once with 128 accumulators, which no call ever has)
#pragma clang loop vectorize(disable) interleave(disable)
    for (int64_t w = 0; w < A.words; ++w) {
        const uint32_t x = mine[w * A.stride];
        const uint32_t *__restrict__ row = rows + w * A.stride;   // wave-uniform: scalar loads
#pragma unroll
        for (int j = 0; j < CS_J; ++j) acc[j] += __popc(x & row[j]);
    }

    const bool a_ok = a < A.M;
    const int64_t ca = A.changes[a];
    const int32_t id_a = A.idx[a];
    const bool dist = A.min_len >= 0;
    const double pa = dist ? (double)A.pos[a] : 0.0;
    const bool partners = LINKS && A.best_in != nullptr;
    const int32_t best_a = partners ? A.best_in[a] : -1;
    uint32_t n_p = 0, n_q = 0, n_zero = 0;
    int32_t my_best = -1, my_partner = INT_MAX;
    uint32_t my_nge = 0;
#pragma unroll
    for (int j = 0; j < CS_J; ++j) {
        const int64_t b = j0 + j;        // (b < stride)
        bool in_p = a_ok && b < A.M && a < b;
        if (dist) in_p = in_p && circ_len((double)A.pos[b], pa, A.g) > A.min_len;
        const int32_t co = acc[j];
        const bool q = in_p && (int64_t)co * A.B >= A.min_lift * ca * (int64_t)A.changes[b];
        const bool ge = q && co >= A.min_co;
        n_p += in_p, n_q += q;
        const unsigned long long bq = __ballot(q);
        if (!bq) continue;
        if (!LINKS) {
            const int bin = co < CS_BINS - 1 ? co : CS_BINS - 1;
            n_zero += q && bin == 0;
            if (q && bin) atomicAdd(&s_hist[bin], 1u);
            my_best = q && co > my_best ? co : my_best;
            my_nge += ge;
            // the J row: every lane with co > 0, and one lane for the rest of them
            if (q && (co > 0 || lane == __ffsll((long long)bq) - 1)) atomicMax(&s_row[j], co);
            const unsigned long long bg = __ballot(ge);
            if (bg && lane == __ffsll((long long)bg) - 1) atomicAdd(&s_nge[j], (uint32_t)__popcll(bg));
        } else {
            const unsigned long long bal = __ballot(ge);
            if (bal) {   // one counter add per wave; the hits take consecutive places
                const int first = __ffsll((long long)bal) - 1;
                unsigned long long base = 0;
                if (lane == first) base = atomicAdd(&A.stat[2], (unsigned long long)__popcll(bal));
                base = __shfl(base, first);
                const unsigned long long at = base + (unsigned long long)__popcll(bal & ((1ull << lane) - 1ull));
                if (ge && at < A.cap) A.la[at] = id_a, A.lb[at] = A.idx[b], A.lco[at] = co;
            }
            if (partners) {
                const int32_t id_b = A.idx[b];
                if (q && co == best_a && id_b < my_partner) my_partner = id_b;
                // the slots ascend with the lanes and the SNPs with the slots: the first matching lane holds the row's smallest partner of this wave
                const unsigned long long bm = __ballot(q && co == A.best_in[b]);
                if (bm && lane == __ffsll((long long)bm) - 1) atomicMin(&s_row[j], id_a);
            }
        }
    }
    for (int o = 32; o; o >>= 1) n_p += __shfl_xor(n_p, o), n_q += __shfl_xor(n_q, o), n_zero += __shfl_xor(n_zero, o);
    if (lane == 0) {
        if (n_p) atomicAdd(&A.stat[0], (unsigned long long)n_p);
        if (n_q) atomicAdd(&A.stat[1], (unsigned long long)n_q);
        if (!LINKS && n_zero) atomicAdd(&s_hist[0], n_zero);
    }
    __syncthreads();
    if (!LINKS) {
        if (my_best >= 0) atomicMax(&A.best[a], my_best);
        if (my_nge) atomicAdd(&A.nge[a], (unsigned long long)my_nge);
        if (tid < CS_J) {   // (a row that met a qualifying pair lies below M)
            if (s_row[tid] >= 0) atomicMax(&A.best[j0 + tid], s_row[tid]);
            if (s_nge[tid]) atomicAdd(&A.nge[j0 + tid], (unsigned long long)s_nge[tid]);
        }
        for (int i = tid; i < CS_BINS; i += CS_THREADS) {
            const uint32_t v = s_hist[i];
            if (v) atomicAdd(&A.hist[i], (unsigned long long)v);
        }
    } else if (partners) {
        if (my_partner != INT_MAX) atomicMin(&A.partner[a], my_partner);
        if (tid < CS_J && s_row[tid] != INT_MAX) atomicMin(&A.partner[j0 + tid], s_row[tid]);
    }
}

}  // namespace ldw

namespace {

// the thresholds of a call, checked
struct CoParams {
    int32_t min_changes = 1, min_co = 0;
    int64_t min_lift = 0;
    double min_len = -1;
};

int co_check_params(const char *who, const CoParams &p) {
    LDW_REQUIRE(p.min_changes >= 1, LDW_ERR_ARG, "%s: min_changes %d (at least 1)", who, (int)p.min_changes);
    LDW_REQUIRE(p.min_co >= 0, LDW_ERR_ARG, "%s: min_co %d (at least 0)", who, (int)p.min_co);
    LDW_REQUIRE(p.min_lift >= 0 && p.min_lift <= CS_MAX_LIFT, LDW_ERR_ARG, "%s: min_lift %lld outside 0..2^20", who, (long long)p.min_lift);
    LDW_REQUIRE(!std::isnan(p.min_len), LDW_ERR_ARG, "%s: min_len is NaN", who);
    return LDW_OK;
}

int co_check_links(const char *who, int64_t cap, const void *a, const void *b, const void *co, const void *count, const void *best, const void *partner) {
    LDW_REQUIRE(count, LDW_ERR_ARG, "%s: null count_out", who);
    LDW_REQUIRE(cap >= 0 && (cap == 0 || (a && b && co)), LDW_ERR_ARG, "%s: cap %lld needs the three lists", who, (long long)cap);
    LDW_REQUIRE(!partner || best, LDW_ERR_ARG, "%s: partner_out needs best_in", who);
    return LDW_OK;
}

// The M slots of a call on the HOST, as the kernel takes them (the debug entries are given them, the tree entries make them), and what comes back over them
struct CoSlots {
    int64_t M = 0, B = 0;
    const int32_t *changes = nullptr, *idx = nullptr, *pos = nullptr;   // [M]; pos may be null where min_len < 0
    double g = 0;
    const int32_t *best_in = nullptr;   // links: [M], or null
};
struct CoScanOut {
    uint64_t *hist;                     // [CS_BINS]
    int32_t *best;                      // [M]
    int64_t *nge;                       // [M]
    int64_t *npairs;                    // [2]
};
struct CoLinksOut {
    int64_t cap;
    int32_t *a, *b, *co;
    int64_t *count;
    int32_t *partner;                   // [M], or null
};

struct CoBufs {   // the working memory of one call
    ParsBufs pars;
    DevBuf bits, changes, idx, pos, best_in, hist, best, nge, partner, stat, la, lb, lco;
    Laps laps;    // in front of the initialisation, behind the pair kernels, behind the copies out
};

// a per-slot int32 array on the device, `stride` long, zero past M
int co_upload_slots(ldw_ctx *c, DevBuf &buf, const int32_t *src, int64_t M, int64_t stride) {
    if (int rc = buf.reserve((size_t)stride * 4)) return rc;
    LDW_HIP(hipMemsetAsync(buf.p, 0, (size_t)stride * 4, c->stream));
    if (M) LDW_HIP(hipMemcpyAsync(buf.p, src, (size_t)M * 4, hipMemcpyHostToDevice, c->stream));
    return LDW_OK;
}

// tile rows of a launch: what a grid dimension holds, LDW_COSCAN_ROWS=k forces k (a test hook, read at every call)
int64_t co_band() { return std::min<int64_t>(budget_or_env(CS_MAX_BAND, "LDW_COSCAN_ROWS"), CS_MAX_BAND); }

// The pair kernels over bits[words][stride] (DEVICE, zero past slot M, stride a multiple of CS_I) and the copies out; scan or links, whichever is given.
// Everything the kernel accumulates into is initialised on the stream in front of it.  Returns with the stream drained: LDW_OK, or LDW_ERR_SIZE with
// *count written.
int co_pairs(ldw_ctx *c, CoBufs &b, const uint32_t *bits, int64_t stride, int64_t words, const CoSlots &s, const CoParams &p, const CoScanOut *scan,
             const CoLinksOut *links, const char *who) {
    const int64_t M = s.M;
    const bool dist = p.min_len >= 0, partners = links && links->partner;
    if (int rc = b.laps.mark(c->stream)) return rc;
    if (int rc = co_upload_slots(c, b.changes, s.changes, M, stride)) return rc;
    if (int rc = co_upload_slots(c, b.idx, s.idx, M, stride)) return rc;
    if (dist)
        if (int rc = co_upload_slots(c, b.pos, s.pos, M, stride)) return rc;
    if (int rc = b.stat.reserve(CS_NSTAT * 8)) return rc;
    LDW_HIP(hipMemsetAsync(b.stat.p, 0, CS_NSTAT * 8, c->stream));
    const size_t m1 = (size_t)std::max<int64_t>(M, 1);
    if (scan) {
        if (int rc = b.hist.reserve(CS_BINS * 8)) return rc;
        if (int rc = b.best.reserve(m1 * 4)) return rc;
        if (int rc = b.nge.reserve(m1 * 8)) return rc;
        LDW_HIP(hipMemsetAsync(b.hist.p, 0, CS_BINS * 8, c->stream));
        LDW_HIP(hipMemsetD32Async((hipDeviceptr_t)b.best.p, -1, m1, c->stream));
        LDW_HIP(hipMemsetAsync(b.nge.p, 0, m1 * 8, c->stream));
    } else {
        const size_t n = (size_t)std::max<int64_t>(links->cap, 1);
        if (int rc = b.la.reserve(n * 4)) return rc;
        if (int rc = b.lb.reserve(n * 4)) return rc;
        if (int rc = b.lco.reserve(n * 4)) return rc;
        if (partners) {
            if (int rc = co_upload_slots(c, b.best_in, s.best_in, M, stride)) return rc;
            if (int rc = b.partner.reserve(m1 * 4)) return rc;
            LDW_HIP(hipMemsetD32Async((hipDeviceptr_t)b.partner.p, INT_MAX, m1, c->stream));
        }
    }
    CoArgs A;
    A.bits = bits, A.stride = stride, A.words = words, A.M = M;
    A.changes = b.changes.as<int32_t>(), A.idx = b.idx.as<int32_t>(), A.pos = dist ? b.pos.as<int32_t>() : nullptr;
    A.g = s.g, A.min_len = dist ? p.min_len : -1.0;
    A.B = s.B, A.min_lift = p.min_lift, A.min_co = p.min_co;
    A.hist = b.hist.as<unsigned long long>(), A.best = b.best.as<int32_t>(), A.nge = b.nge.as<unsigned long long>();
    A.best_in = partners ? b.best_in.as<int32_t>() : nullptr, A.partner = b.partner.as<int32_t>();
    A.cap = links ? (unsigned long long)links->cap : 0ull;
    A.la = b.la.as<int32_t>(), A.lb = b.lb.as<int32_t>(), A.lco = b.lco.as<int32_t>();
    A.stat = b.stat.as<unsigned long long>();
    const int64_t TI = ceil_div(M, CS_I), TJ = ceil_div(M, CS_J), band = co_band();
    for (int64_t r0 = 0; r0 < TI && M >= 2; r0 += band) {
        const int64_t rows = std::min<int64_t>(band, TI - r0);
        A.ti0 = r0, A.tj0 = r0 * (CS_I / CS_J);   // the first tile column that holds a slot above the band's first
        const dim3 grid((unsigned)(TJ - A.tj0), (unsigned)rows);
        if (links) hipLaunchKernelGGL(k_coscan<true>, grid, dim3(CS_THREADS), 0, c->stream, A);
        else hipLaunchKernelGGL(k_coscan<false>, grid, dim3(CS_THREADS), 0, c->stream, A);
        LDW_HIP(hipGetLastError());
    }
    if (int rc = b.laps.mark(c->stream)) return rc;
    unsigned long long st[CS_NSTAT];
    LDW_HIP(hipMemcpyAsync(st, b.stat.p, sizeof st, hipMemcpyDeviceToHost, c->stream));
    int rc = LDW_OK;
    if (scan) {
        LDW_HIP(hipMemcpyAsync(scan->hist, b.hist.p, CS_BINS * 8, hipMemcpyDeviceToHost, c->stream));
        if (M) LDW_HIP(hipMemcpyAsync(scan->best, b.best.p, (size_t)M * 4, hipMemcpyDeviceToHost, c->stream));
        if (M) LDW_HIP(hipMemcpyAsync(scan->nge, b.nge.p, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipStreamSynchronize(c->stream));
        scan->npairs[0] = (int64_t)st[0], scan->npairs[1] = (int64_t)st[1];
    } else {
        if (partners && M) LDW_HIP(hipMemcpyAsync(links->partner, b.partner.p, (size_t)M * 4, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipStreamSynchronize(c->stream));
        if (partners)
            for (int64_t i = 0; i < M; ++i)
                if (links->partner[i] == INT_MAX) links->partner[i] = -1;
        const int64_t n = (int64_t)st[2];
        *links->count = n;
        if (!(links->cap == 0 && !links->a)) {   // (else a pure count)
            if (n > links->cap) {
                set_error("%s: %lld pairs qualify with co >= min_co, cap %lld", who, (long long)n, (long long)links->cap);
                rc = LDW_ERR_SIZE;
            } else if (n) {
                LDW_HIP(hipMemcpyAsync(links->a, b.la.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
                LDW_HIP(hipMemcpyAsync(links->b, b.lb.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
                LDW_HIP(hipMemcpyAsync(links->co, b.lco.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
                LDW_HIP(hipStreamSynchronize(c->stream));
            }
        }
    }
    if (int rc2 = b.laps.mark(c->stream)) return rc2;
    LDW_HIP(hipStreamSynchronize(c->stream));
    return rc;
}

// ldw_ctx_last_timing: [0] the pair kernels (with the initialisation in front of them), [1] the parsimony passes and gathers, [2] the copies out, [3] their sum
int co_timing(ldw_ctx *c, const CoBufs &b, double pars_ms, double copies_ms) {
    double ms[2] = {0, 0};
    if (int rc = b.laps.sums(2, ms)) return rc;
    c->last_ms[0] = ms[0], c->last_ms[1] = pars_ms, c->last_ms[2] = ms[1] + copies_ms, c->last_ms[3] = ms[0] + pars_ms + ms[1] + copies_ms;
    return LDW_OK;
}

// What both tree entries do in front of the pair kernels: the refusals, the scores of all L SNPs, the eligible list, its bitmaps.  Leaves bits[words][stride] in
// b.bits and the slots in the vectors; pars_ms / copies_ms: the passes with their gathers, the copies of the scores.
struct CoTree {
    std::vector<int32_t> score, idx, changes, pos;
    int64_t stride = 0, words = 0;
    double pars_ms = 0, copies_ms = 0;
};

int co_tree_prepare(ldw_ctx *c, CoBufs &b, const char *who, const int32_t *parent, const int32_t *tip_seq, int64_t nodes, int32_t gap_mode, const CoParams &p, CoTree &T) {
    LDW_REQUIRE(have_alignment(c), LDW_ERR_STATE, "%s: no alignment resident: set the alignment first", who);
    if (int rc = co_check_params(who, p)) return rc;
    LDW_REQUIRE(!(p.min_len >= 0) || (c->meta.have_meta && (int64_t)c->meta.h_POS.size() == c->L), LDW_ERR_STATE,
                "%s: min_len >= 0 needs the SNP positions (ldw_set_snp_meta)", who);
    ParsTree t;
    if (int rc = pars_check_tree(c, who, parent, tip_seq, nodes, gap_mode, t)) return rc;
    LDW_REQUIRE(nodes <= CS_MAX_NODES, LDW_ERR_ARG, "%s: %lld nodes (at most 2^21)", who, (long long)nodes);
    const int64_t L = c->L;
    T.score.resize((size_t)L);
    {
        ParsRun run{c, b.pars, t, gap_mode};
        if (int rc = run.start(parent, L, nullptr, true, false)) return rc;
        if (int rc = run.chunks(L, false, true, false, nullptr, 0, [&](int64_t j0, int64_t count) {
                LDW_HIP(hipMemcpyAsync(T.score.data() + j0, b.pars.score.p, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
                return (int)LDW_OK;
            }))
            return rc;
        LDW_HIP(hipStreamSynchronize(c->stream));
        double ms[3] = {0, 0, 0};
        if (int rc = run.lap_sums(ms)) return rc;
        T.pars_ms += ms[0] + ms[1], T.copies_ms += ms[2];
    }
    for (int64_t i = 0; i < L; ++i)
        if (T.score[(size_t)i] >= p.min_changes) T.idx.push_back((int32_t)i);
    const int64_t M = (int64_t)T.idx.size();
    T.changes.resize((size_t)M);
    for (int64_t k = 0; k < M; ++k) T.changes[(size_t)k] = T.score[(size_t)T.idx[(size_t)k]];
    if (p.min_len >= 0) {
        T.pos.resize((size_t)M);
        for (int64_t k = 0; k < M; ++k) T.pos[(size_t)k] = c->meta.h_POS[(size_t)T.idx[(size_t)k]];
    }
    T.stride = round_up(std::max<int64_t>(M, 1), CS_I), T.words = ceil_div(nodes, 32);
    if (M < 2) return LDW_OK;   // no pair: no bitmap is read
    if (int rc = b.bits.reserve((size_t)T.words * (size_t)T.stride * 4)) return rc;
    LDW_HIP(hipMemsetAsync(b.bits.p, 0, (size_t)T.words * (size_t)T.stride * 4, c->stream));   // the slots past M
    ParsRun run{c, b.pars, t, gap_mode};
    if (int rc = run.start(parent, M, T.idx.data(), false, true)) return rc;
    if (int rc = run.chunks(M, true, false, true, b.bits.as<uint32_t>(), T.stride, [](int64_t, int64_t) { return (int)LDW_OK; })) return rc;
    LDW_HIP(hipStreamSynchronize(c->stream));
    double ms[3] = {0, 0, 0};
    if (int rc = run.lap_sums(ms)) return rc;
    T.pars_ms += ms[0] + ms[1] + ms[2];
    return LDW_OK;
}

int tree_scan_run(ldw_ctx *c, CoBufs &b, const int32_t *parent, const int32_t *tip_seq, int64_t nodes, int32_t gap_mode, const CoParams &p, int32_t *changes_out,
                  uint64_t *hist_out, int32_t *best_out, int64_t *nge_out, int64_t *npairs_out) {
    const char *who = "ldw_tree_cochange_scan";
    LDW_REQUIRE(changes_out && hist_out && best_out && nge_out && npairs_out, LDW_ERR_ARG, "%s: output is null", who);
    CoTree T;
    if (int rc = co_tree_prepare(c, b, who, parent, tip_seq, nodes, gap_mode, p, T)) return rc;
    const int64_t L = c->L, M = (int64_t)T.idx.size();
    std::vector<int32_t> best((size_t)std::max<int64_t>(M, 1));
    std::vector<int64_t> nge((size_t)std::max<int64_t>(M, 1));
    CoSlots s;
    s.M = M, s.B = nodes - 1, s.changes = T.changes.data(), s.idx = T.idx.data(), s.pos = T.pos.data(), s.g = c->meta.g;
    const CoScanOut out{hist_out, best.data(), nge.data(), npairs_out};
    if (int rc = co_pairs(c, b, b.bits.as<uint32_t>(), T.stride, T.words, s, p, &out, nullptr, who)) return rc;
    for (int64_t i = 0; i < L; ++i) changes_out[i] = T.score[(size_t)i], best_out[i] = -1, nge_out[i] = 0;
    for (int64_t k = 0; k < M; ++k) best_out[T.idx[(size_t)k]] = best[(size_t)k], nge_out[T.idx[(size_t)k]] = nge[(size_t)k];
    return co_timing(c, b, T.pars_ms, T.copies_ms);
}

int tree_links_run(ldw_ctx *c, CoBufs &b, const int32_t *parent, const int32_t *tip_seq, int64_t nodes, int32_t gap_mode, const CoParams &p, const int32_t *best_in,
                   int64_t cap, int32_t *a_out, int32_t *b_out, int32_t *co_out, int64_t *count_out, int32_t *partner_out) {
    const char *who = "ldw_tree_cochange_links";
    if (int rc = co_check_links(who, cap, a_out, b_out, co_out, count_out, best_in, partner_out)) return rc;
    CoTree T;
    if (int rc = co_tree_prepare(c, b, who, parent, tip_seq, nodes, gap_mode, p, T)) return rc;
    const int64_t L = c->L, M = (int64_t)T.idx.size();
    std::vector<int32_t> bin, part;
    if (partner_out) {
        bin.resize((size_t)std::max<int64_t>(M, 1)), part.resize((size_t)std::max<int64_t>(M, 1));
        for (int64_t k = 0; k < M; ++k) bin[(size_t)k] = best_in[T.idx[(size_t)k]];
    }
    CoSlots s;
    s.M = M, s.B = nodes - 1, s.changes = T.changes.data(), s.idx = T.idx.data(), s.pos = T.pos.data(), s.g = c->meta.g;
    s.best_in = partner_out ? bin.data() : nullptr;
    const CoLinksOut out{cap, a_out, b_out, co_out, count_out, partner_out ? part.data() : nullptr};
    const int rc = co_pairs(c, b, b.bits.as<uint32_t>(), T.stride, T.words, s, p, nullptr, &out, who);
    if (rc != LDW_OK && rc != LDW_ERR_SIZE) return rc;
    if (partner_out) {
        for (int64_t i = 0; i < L; ++i) partner_out[i] = -1;
        for (int64_t k = 0; k < M; ++k) partner_out[T.idx[(size_t)k]] = part[(size_t)k];
    }
    if (int rc2 = co_timing(c, b, T.pars_ms, T.copies_ms)) return rc2;
    return rc;
}

// ---- the debug entries: the slots and their bitmaps from the HOST -----------------------------------------------------------------------------------------
int debug_check(const char *who, const uint32_t *bits, int64_t words, int64_t M, const int32_t *changes, const int32_t *idx, const int32_t *pos, double g, int64_t B,
                const CoParams &p) {
    if (int rc = co_check_params(who, p)) return rc;
    LDW_REQUIRE(M >= 0 && M <= (1ll << 24) && words >= 1 && words <= CS_MAX_NODES / 32, LDW_ERR_ARG, "%s: M outside 0..2^24 or words outside 1..2^16", who);
    LDW_REQUIRE(M == 0 || (bits && changes && idx), LDW_ERR_ARG, "%s: null argument", who);
    LDW_REQUIRE(B >= 1 && B < CS_MAX_NODES, LDW_ERR_ARG, "%s: B outside 1..2^21 - 1", who);
    if (p.min_len >= 0) LDW_REQUIRE((pos || M == 0) && std::isfinite(g) && g > 0, LDW_ERR_ARG, "%s: min_len >= 0 needs pos and a positive g", who);
    for (int64_t i = 0; i < M; ++i) {
        LDW_REQUIRE(changes[i] >= 0 && changes[i] < CS_MAX_NODES, LDW_ERR_ARG, "%s: changes[%lld] outside 0..2^21 - 1", who, (long long)i);
        LDW_REQUIRE(idx[i] >= 0 && idx[i] < INT_MAX && (i == 0 || idx[i] > idx[i - 1]), LDW_ERR_ARG, "%s: idx[%lld] negative or not above idx[%lld]", who, (long long)i,
                    (long long)(i - 1));
    }
    return LDW_OK;
}

// bits[words][M] (HOST) into bits[words][stride] on the device, zero past M
int debug_bits(ldw_ctx *c, CoBufs &b, const uint32_t *bits, int64_t words, int64_t M, int64_t stride) {
    if (int rc = b.bits.reserve((size_t)words * (size_t)stride * 4)) return rc;
    LDW_HIP(hipMemsetAsync(b.bits.p, 0, (size_t)words * (size_t)stride * 4, c->stream));
    if (M) LDW_HIP(hipMemcpy2DAsync(b.bits.p, (size_t)stride * 4, bits, (size_t)M * 4, (size_t)M * 4, (size_t)words, hipMemcpyHostToDevice, c->stream));
    return LDW_OK;
}

}  // namespace

extern "C" {

int ldw_tree_cochange_scan(ldw_ctx *c, const int32_t *parent, const int32_t *tip_seq, int64_t nodes, int32_t gap_mode, int32_t min_changes, int32_t min_co, int64_t min_lift,
                           double min_len, int32_t *changes_out, uint64_t *hist_out, int32_t *best_out, int64_t *nge_out, int64_t *npairs_out) {
    CoParams p;
    p.min_changes = min_changes, p.min_co = min_co, p.min_lift = min_lift, p.min_len = min_len;
    return scoped_call<CoBufs>(c, [&](CoBufs &b) { return tree_scan_run(c, b, parent, tip_seq, nodes, gap_mode, p, changes_out, hist_out, best_out, nge_out, npairs_out); });
}

int ldw_tree_cochange_links(ldw_ctx *c, const int32_t *parent, const int32_t *tip_seq, int64_t nodes, int32_t gap_mode, int32_t min_changes, int32_t min_co, int64_t min_lift,
                            double min_len, const int32_t *best_in, int64_t cap, int32_t *a_out, int32_t *b_out, int32_t *co_out, int64_t *count_out, int32_t *partner_out) {
    CoParams p;
    p.min_changes = min_changes, p.min_co = min_co, p.min_lift = min_lift, p.min_len = min_len;
    return scoped_call<CoBufs>(
        c, [&](CoBufs &b) { return tree_links_run(c, b, parent, tip_seq, nodes, gap_mode, p, best_in, cap, a_out, b_out, co_out, count_out, partner_out); });
}

int ldw_debug_cochange_scan(ldw_ctx *c, const uint32_t *bits, int64_t words, int64_t M, const int32_t *changes, const int32_t *idx, const int32_t *pos, double g, int64_t B,
                            int32_t min_co, int64_t min_lift, double min_len, uint64_t *hist_out, int32_t *best_out, int64_t *nge_out, int64_t *npairs_out) {
    const char *who = "ldw_debug_cochange_scan";
    CoParams p;
    p.min_co = min_co, p.min_lift = min_lift, p.min_len = min_len;
    return scoped_call<CoBufs>(c, [&](CoBufs &b) {
        if (int rc = debug_check(who, bits, words, M, changes, idx, pos, g, B, p)) return rc;
        LDW_REQUIRE(hist_out && npairs_out && (M == 0 || (best_out && nge_out)), LDW_ERR_ARG, "%s: output is null", who);
        if (int rc = join_prepare(c)) return rc;
        const int64_t stride = round_up(std::max<int64_t>(M, 1), CS_I);
        if (int rc = debug_bits(c, b, bits, words, M, stride)) return rc;
        CoSlots s;
        s.M = M, s.B = B, s.changes = changes, s.idx = idx, s.pos = pos, s.g = g;
        const CoScanOut out{hist_out, best_out, nge_out, npairs_out};
        return co_pairs(c, b, b.bits.as<uint32_t>(), stride, words, s, p, &out, nullptr, who);
    });
}

int ldw_debug_cochange_links(ldw_ctx *c, const uint32_t *bits, int64_t words, int64_t M, const int32_t *changes, const int32_t *idx, const int32_t *pos, double g, int64_t B,
                             int32_t min_co, int64_t min_lift, double min_len, const int32_t *best_in, int64_t cap, int32_t *a_out, int32_t *b_out, int32_t *co_out,
                             int64_t *count_out, int32_t *partner_out) {
    const char *who = "ldw_debug_cochange_links";
    CoParams p;
    p.min_co = min_co, p.min_lift = min_lift, p.min_len = min_len;
    return scoped_call<CoBufs>(c, [&](CoBufs &b) {
        if (int rc = debug_check(who, bits, words, M, changes, idx, pos, g, B, p)) return rc;
        if (int rc = co_check_links(who, cap, a_out, b_out, co_out, count_out, best_in, partner_out)) return rc;
        if (int rc = join_prepare(c)) return rc;
        const int64_t stride = round_up(std::max<int64_t>(M, 1), CS_I);
        if (int rc = debug_bits(c, b, bits, words, M, stride)) return rc;
        CoSlots s;
        s.M = M, s.B = B, s.changes = changes, s.idx = idx, s.pos = pos, s.g = g, s.best_in = partner_out ? best_in : nullptr;
        const CoLinksOut out{cap, a_out, b_out, co_out, count_out, partner_out};
        return co_pairs(c, b, b.bits.as<uint32_t>(), stride, words, s, p, nullptr, &out, who);
    });
}

}  // extern "C"
