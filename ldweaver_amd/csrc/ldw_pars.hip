// Maximum parsimony on a given tree: ldw_tree_parsimony scores every SNP column of the resident alignment, ldw_tree_states gives the
// stated most-parsimonious reconstruction of chosen columns at every node, ldw_tree_cochanges counts the branches on which both SNPs of a pair change.
//
// The walk over the nodes is the same for every SNP, so a lane owns four SNPs — the bytes of a dword — and everything that names a node is wave-uniform.
// The working memory of a chunk of C SNPs is sets[node][Cpad] (Cpad = C rounded up to PARS_TILE), a byte per SNP: bit s stands for state s.
//   k_pars_tips   the tips' sets, gathered from states[L][Npad] through the tips' sequences (sorted, so a row is read front to back) and transposed in
//                 LDS: rows of the alignment come in along the sequences, rows of sets go out along the SNPs; the states seen at the tips are OR-ed into seen[];
//   k_pars_up     Hartigan's rule from the last node to the first, the children read once each through the CSR of the tree; counts live in registers, so
//                 arity has no limit; the score and min_changes of the lane's four SNPs;
//   k_pars_down   node 0 takes the lowest state of its set, every other node its parent's state where its set holds it, else its set's lowest: sets[] turns
//                 into one-hot states in place; with a bitmap, bit v of a SNP's row is set where branch v changes;
//   k_pars_emit   sets[node][slot] -> state[slot][node] (0..4), transposed in LDS;
//   k_pars_pairs  a thread per pair: popcounts of the two bitmaps and of their AND.
// A lane reads only what it wrote itself (its own dword column of sets), so the passes need no barrier between nodes.
#include <algorithm>
#include <vector>

#include "ldw_internal.h"
#include "ldw_pars.h"
#include "ldw_seq_plan.h"

using namespace ldw;

namespace ldw {

constexpr int PARS_TILE = 256;          // SNPs of a gather tile = the unit Cpad is rounded to (64 dwords: a wave's row of sets)
constexpr int PARS_TIPS = 64;           // tips of a gather tile
constexpr int PARS_LDS_ROW = PARS_TILE + 4;   // bytes: rows 65 dwords apart, so the 64 tips of a read step fall into 64 banks
constexpr int PARS_WAVE = 64;           // threads of a workgroup of the two passes: one wave, so that few SNPs still spread over the CUs
constexpr int64_t PARS_BUDGET = (int64_t)1 << 30;   // bytes of sets[] a chunk may take
constexpr int64_t PARS_MAX_CHUNK = (int64_t)1 << 21;   // SNPs of a chunk at most: the second grid dimension of the gather and of the transpose stays below 2^16

// per byte of x (every byte below 0x80): 0xFF where the byte is not zero
__device__ __forceinline__ uint32_t pars_nonzero_bytes(uint32_t x) { return (((x + 0x7F7F7F7Fu) & 0x80808080u) >> 7) * 0xFFu; }
// per byte of x (no byte zero): its lowest set bit
__device__ __forceinline__ uint32_t pars_low_bits(uint32_t x) { return x & ~(x - 0x01010101u); }

// tile (blockIdx.x: 64 tips, blockIdx.y: 256 SNP slots of the chunk).  snp: the SNP of every slot, or null for first + slot.  Slots past `count` get the
// set {A}: never read back, but no lane ever meets an empty set.
__global__ __launch_bounds__(256) void k_pars_tips(const uint8_t *__restrict__ states, int64_t Npad, const int32_t *__restrict__ tip_seq, const int32_t *__restrict__ tip_node,
                                                   int64_t tips, const int32_t *__restrict__ snp, int64_t first, int64_t count, int32_t gap_mode,
                                                   uint32_t *__restrict__ sets, int64_t stride4, uint32_t *__restrict__ seen) {
    __shared__ __attribute__((aligned(4))) uint8_t sh[PARS_TIPS * PARS_LDS_ROW];
    const int tid = threadIdx.x, lo = tid & 63, hi = tid >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * PARS_TIPS, j0 = (int64_t)blockIdx.y * PARS_TILE;
    const int64_t t = t0 + lo;
    if (t < tips) {
        const int64_t seq = tip_seq[t];
        for (int it = 0; it < PARS_TILE / 4; ++it) {
            const int jl = it * 4 + hi;
            const int64_t j = j0 + jl;
            uint8_t m = 1;
            if (j < count) {
                const int64_t l = snp ? (int64_t)snp[j] : first + j;
                const uint32_t raw = states[l * Npad + seq], s = raw < 4u ? raw : 4u;
                m = (s == 4 && gap_mode == 0) ? (uint8_t)0x0F : (uint8_t)(1u << s);
            }
            sh[lo * PARS_LDS_ROW + jl] = m;
        }
    }
    __syncthreads();
    uint32_t acc = 0;
    for (int it = 0; it < PARS_TIPS / 4; ++it) {
        const int tl = it * 4 + hi;
        if (t0 + tl >= tips) break;
        const uint32_t w = *reinterpret_cast<const uint32_t *>(&sh[tl * PARS_LDS_ROW + 4 * lo]);
        sets[(int64_t)tip_node[t0 + tl] * stride4 + j0 / 4 + lo] = w;
        // a wildcard tip shows no state (a set of one state is never 0x0F)
        acc |= w & pars_nonzero_bytes(w ^ 0x0F0F0F0Fu);
    }
    if (acc) atomicOr(&seen[j0 / 4 + lo], acc);
}

// score_out / min_out [4 stride4] (may be null: the sets alone are wanted)
__global__ __launch_bounds__(PARS_WAVE) void k_pars_up(uint32_t *__restrict__ sets, int64_t stride4, int64_t nodes, const int32_t *__restrict__ child_ptr,
                                                       const int32_t *__restrict__ child_idx, const uint32_t *__restrict__ seen, int32_t *__restrict__ score_out,
                                                       int32_t *__restrict__ min_out) {
    const int64_t d = (int64_t)blockIdx.x * PARS_WAVE + threadIdx.x;
    int32_t score[4] = {0, 0, 0, 0};
    for (int64_t v = nodes - 1; v >= 0; --v) {
        const int32_t p0 = child_ptr[v], p1 = child_ptr[v + 1], arity = p1 - p0;
        if (arity == 0) continue;
        uint32_t out;
        if (arity == 2) {   // Fitch: the intersection where there is one, else the union
            const uint32_t a = sets[(int64_t)child_idx[p0] * stride4 + d], b = sets[(int64_t)child_idx[p0 + 1] * stride4 + d];
            const uint32_t both = a & b, m = pars_nonzero_bytes(both);
            out = (both & m) | ((a | b) & ~m);
#pragma unroll
            for (int k = 0; k < 4; ++k) score[k] += (int32_t)((~m >> (8 * k)) & 1u);
        } else {
            int32_t c[4][5];
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int s = 0; s < 5; ++s) c[k][s] = 0;
            for (int32_t p = p0; p < p1; ++p) {
                const uint32_t x = sets[(int64_t)child_idx[p] * stride4 + d];
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int s = 0; s < 5; ++s) c[k][s] += (int32_t)((x >> (8 * k + s)) & 1u);
            }
            out = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int32_t K = c[k][0];
#pragma unroll
                for (int s = 1; s < 5; ++s) K = c[k][s] > K ? c[k][s] : K;
#pragma unroll
                for (int s = 0; s < 5; ++s) out |= c[k][s] == K ? 1u << (8 * k + s) : 0u;
                score[k] += arity - K;
            }
        }
        sets[v * stride4 + d] = out;
    }
    if (score_out) {
        const uint32_t sn = seen[d];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int32_t n = __popc((sn >> (8 * k)) & 0xFFu);
            score_out[4 * d + k] = score[k];
            min_out[4 * d + k] = n > 0 ? n - 1 : 0;
        }
    }
}

// bits (may be null): [words][bit_stride] uint32, word w of slot j at bits[w bit_stride + j]; this chunk's slots start at slot0, `count` of them are real
__global__ __launch_bounds__(PARS_WAVE) void k_pars_down(uint32_t *__restrict__ sets, int64_t stride4, int64_t nodes, const int32_t *__restrict__ parent,
                                                         uint32_t *__restrict__ bits, int64_t bit_stride, int64_t slot0, int64_t count) {
    const int64_t d = (int64_t)blockIdx.x * PARS_WAVE + threadIdx.x;
    sets[d] = pars_low_bits(sets[d]);
    uint32_t word[4] = {0, 0, 0, 0};
    for (int64_t v = 1; v < nodes; ++v) {
        const uint32_t up = sets[(int64_t)parent[v] * stride4 + d], mine = sets[v * stride4 + d];
        const uint32_t keep = pars_nonzero_bytes(mine & up);
        sets[v * stride4 + d] = (up & keep) | (pars_low_bits(mine) & ~keep);
        if (bits) {
#pragma unroll
            for (int k = 0; k < 4; ++k) word[k] |= ((~keep >> (8 * k)) & 1u) << (v & 31);
            if ((v & 31) == 31 || v == nodes - 1) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (4 * d + k < count) bits[(v >> 5) * bit_stride + slot0 + 4 * d + k] = word[k];
                    word[k] = 0;
                }
            }
        }
    }
}

// tile of 64 nodes x 64 slots: out[slot][node] = the state whose bit sets[node][slot] holds
__global__ __launch_bounds__(256) void k_pars_emit(const uint8_t *__restrict__ sets, int64_t stride, int64_t nodes, int64_t count, uint8_t *__restrict__ out) {
    __shared__ uint8_t sh[64][65];
    const int lo = threadIdx.x & 63, hi = threadIdx.x >> 6;
    const int64_t v0 = (int64_t)blockIdx.x * 64, j0 = (int64_t)blockIdx.y * 64;
    for (int it = 0; it < 16; ++it) {
        const int vl = it * 4 + hi;
        if (v0 + vl < nodes && j0 + lo < count) sh[vl][lo] = (uint8_t)(__ffs((int)sets[(v0 + vl) * stride + j0 + lo]) - 1);
    }
    __syncthreads();
    for (int it = 0; it < 16; ++it) {
        const int jl = it * 4 + hi;
        if (v0 + lo < nodes && j0 + jl < count) out[(j0 + jl) * nodes + v0 + lo] = sh[lo][jl];
    }
}

__global__ __launch_bounds__(256) void k_pars_pairs(const uint32_t *__restrict__ bits, int64_t bit_stride, int64_t words, const int32_t *__restrict__ slot_a,
                                                    const int32_t *__restrict__ slot_b, int64_t K, int32_t *__restrict__ ca, int32_t *__restrict__ cb,
                                                    int32_t *__restrict__ co) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= K) return;
    const int64_t a = slot_a[i], b = slot_b[i];
    int32_t na = 0, nb = 0, nab = 0;
    for (int64_t w = 0; w < words; ++w) {
        const uint32_t x = bits[w * bit_stride + a], y = bits[w * bit_stride + b];
        na += __popc(x), nb += __popc(y), nab += __popc(x & y);
    }
    ca[i] = na, cb[i] = nb, co[i] = nab;
}

}  // namespace ldw

int ldw::pars_check_tree(const ldw_ctx *c, const char *who, const int32_t *parent, const int32_t *tip_seq, int64_t nodes, int32_t gap_mode, ParsTree &t) {
    LDW_REQUIRE(parent && tip_seq, LDW_ERR_ARG, "%s: parent or tip_seq is null", who);
    LDW_REQUIRE(gap_mode == 0 || gap_mode == 1, LDW_ERR_ARG, "%s: gap_mode %d (0: N is missing, 1: N is a state)", who, (int)gap_mode);
    LDW_REQUIRE(nodes >= 2, LDW_ERR_ARG, "%s: %lld nodes (a tree needs at least 2)", who, (long long)nodes);
    LDW_REQUIRE(nodes < (1ll << 30), LDW_ERR_ARG, "%s: too many nodes", who);
    LDW_REQUIRE(parent[0] == -1, LDW_ERR_ARG, "%s: parent[0] = %d (node 0 is the root: -1)", who, (int)parent[0]);
    t.nodes = nodes;
    t.child_ptr.assign((size_t)nodes + 1, 0);
    for (int64_t v = 1; v < nodes; ++v) {
        LDW_REQUIRE(parent[v] >= 0 && parent[v] < v, LDW_ERR_ARG, "%s: parent[%lld] = %d (a parent comes before its node: 0..%lld)", who, (long long)v,
                    (int)parent[v], (long long)(v - 1));
        ++t.child_ptr[(size_t)parent[v] + 1];
    }
    for (int64_t v = 0; v < nodes; ++v) t.child_ptr[(size_t)v + 1] += t.child_ptr[(size_t)v];
    t.child_idx.resize((size_t)nodes - 1);
    {
        std::vector<int32_t> at(t.child_ptr.begin(), t.child_ptr.end() - 1);
        for (int64_t v = 1; v < nodes; ++v) t.child_idx[(size_t)at[(size_t)parent[v]]++] = (int32_t)v;
    }
    std::vector<int32_t> user((size_t)c->N, -1);   // the tip that holds a sequence
    std::vector<std::pair<int32_t, int32_t>> tp;
    for (int64_t v = 0; v < nodes; ++v) {
        if (t.child_ptr[(size_t)v + 1] > t.child_ptr[(size_t)v]) {
            LDW_REQUIRE(tip_seq[v] == -1, LDW_ERR_ARG, "%s: node %lld has children but tip_seq %d (-1 for such a node)", who, (long long)v, (int)tip_seq[v]);
            continue;
        }
        const int32_t s = tip_seq[v];
        LDW_REQUIRE(s >= 0 && s < c->N, LDW_ERR_ARG, "%s: tip node %lld names sequence %d (the alignment has 0..%lld)", who, (long long)v, (int)s,
                    (long long)(c->N - 1));
        LDW_REQUIRE(user[(size_t)s] < 0, LDW_ERR_ARG, "%s: tip nodes %d and %lld both name sequence %d", who, (int)user[(size_t)s], (long long)v, (int)s);
        user[(size_t)s] = (int32_t)v;
        tp.emplace_back(s, (int32_t)v);
    }
    LDW_REQUIRE(tp.size() >= 2, LDW_ERR_ARG, "%s: a tree of %lld tips (at least 2)", who, (long long)tp.size());
    std::sort(tp.begin(), tp.end());
    t.tips = (int64_t)tp.size();
    t.tip_seq.resize(tp.size()), t.tip_node.resize(tp.size());
    for (size_t k = 0; k < tp.size(); ++k) t.tip_seq[k] = tp[k].first, t.tip_node[k] = tp[k].second;
    return LDW_OK;
}

namespace {

// SNPs of a chunk: what PARS_BUDGET bytes of sets hold, LDW_PARS_CHUNK=k forces k (a test hook, read at every call); never more than `total`
int64_t pars_chunk(int64_t nodes, int64_t total) {
    const int64_t C = ldw::budget_or_env(std::max<int64_t>(PARS_TILE, PARS_BUDGET / nodes / PARS_TILE * PARS_TILE), "LDW_PARS_CHUNK");
    return std::min<int64_t>(std::min<int64_t>(C, PARS_MAX_CHUNK), total);
}

}  // namespace

// ParsRun (ldw_pars.h)
int ldw::ParsRun::start(const int32_t *parent, int64_t total, const int32_t *snp, bool want_score, bool down) {
    C = pars_chunk(t.nodes, total), Cpad = round_up(C, PARS_TILE), stride4 = Cpad / 4;
    int rc = LDW_OK;
    if ((rc = b.sets.reserve((size_t)t.nodes * (size_t)Cpad)) || (rc = b.seen.reserve((size_t)Cpad)) ||
        (want_score && ((rc = b.score.reserve((size_t)Cpad * 4)) || (rc = b.minch.reserve((size_t)Cpad * 4)))))
        return rc;
    if ((rc = ldw::upload(c, b.child_ptr, t.child_ptr.data(), t.child_ptr.size())) || (rc = ldw::upload(c, b.child_idx, t.child_idx.data(), t.child_idx.size())) ||
        (rc = ldw::upload(c, b.tip_seq, t.tip_seq.data(), t.tip_seq.size())) || (rc = ldw::upload(c, b.tip_node, t.tip_node.data(), t.tip_node.size())))
        return rc;
    if (down && (rc = ldw::upload(c, b.parent, parent, (size_t)t.nodes))) return rc;
    if (snp && (rc = ldw::upload(c, b.snp, snp, (size_t)total))) return rc;
    return LDW_OK;
}

int ldw::ParsRun::chunks(int64_t total, bool have_snp, bool want_score, bool down, uint32_t *bits, int64_t bit_stride, const std::function<int(int64_t, int64_t)> &after_chunk) {
    uint32_t *sets = b.sets.as<uint32_t>(), *seen = b.seen.as<uint32_t>();
    for (int64_t j0 = 0; j0 < total; j0 += C) {
        const int64_t count = std::min<int64_t>(C, total - j0);
        if (int rc = laps.mark(c->stream)) return rc;
        LDW_HIP(hipMemsetAsync(seen, 0, (size_t)Cpad, c->stream));
        hipLaunchKernelGGL(k_pars_tips, dim3((unsigned)((t.tips + PARS_TIPS - 1) / PARS_TIPS), (unsigned)(Cpad / PARS_TILE)), dim3(256), 0, c->stream,
                           c->states.as<uint8_t>(), c->Npad, b.tip_seq.as<int32_t>(), b.tip_node.as<int32_t>(), t.tips,
                           have_snp ? b.snp.as<int32_t>() + j0 : (const int32_t *)nullptr, j0, count, gap_mode, sets, stride4, seen);
        LDW_HIP(hipGetLastError());
        if (int rc = laps.mark(c->stream)) return rc;
        hipLaunchKernelGGL(k_pars_up, dim3((unsigned)(stride4 / PARS_WAVE)), dim3(PARS_WAVE), 0, c->stream, sets, stride4, t.nodes, b.child_ptr.as<int32_t>(),
                           b.child_idx.as<int32_t>(), seen, want_score ? b.score.as<int32_t>() : (int32_t *)nullptr,
                           want_score ? b.minch.as<int32_t>() : (int32_t *)nullptr);
        if (down)
            hipLaunchKernelGGL(k_pars_down, dim3((unsigned)(stride4 / PARS_WAVE)), dim3(PARS_WAVE), 0, c->stream, sets, stride4, t.nodes, b.parent.as<int32_t>(),
                               bits, bit_stride, j0, count);
        LDW_HIP(hipGetLastError());
        if (int rc = laps.mark(c->stream)) return rc;
        if (int rc = after_chunk(j0, count)) return rc;
    }
    return laps.mark(c->stream);
}

// after the stream has drained
int ldw::ParsRun::finish() {
    double ms[3] = {0, 0, 0};
    if (int rc = lap_sums(ms)) return rc;
    c->last_ms[0] = ms[1];   // the passes
    c->last_ms[1] = ms[0];   // the gathers
    c->last_ms[2] = ms[2];   // what followed a chunk: the copies out, the transposes, the pairs
    c->last_ms[3] = ms[0] + ms[1] + ms[2];
    return LDW_OK;
}

namespace {

int pars_check_snps(const ldw_ctx *c, const char *who, const char *what, const int32_t *idx, int64_t n) {
    const int64_t k = ldw::first_bad_index(idx, n, c->L);
    LDW_REQUIRE(k < 0, LDW_ERR_ARG, "%s: %s[%lld] = %d (the alignment has SNPs 0..%lld)", who, what, (long long)k, (int)idx[k], (long long)(c->L - 1));
    return LDW_OK;
}

int parsimony_run(ldw_ctx *c, const int32_t *parent, const int32_t *tip_seq, int64_t nodes, int32_t gap_mode, int32_t *score_out, int32_t *min_out, ParsBufs &b) {
    const char *who = "ldw_tree_parsimony";
    LDW_REQUIRE(ldw::have_alignment(c), LDW_ERR_STATE, "%s: no alignment resident: set the alignment first", who);
    LDW_REQUIRE(score_out && min_out, LDW_ERR_ARG, "%s: output is null", who);
    ParsTree t;
    if (int rc = pars_check_tree(c, who, parent, tip_seq, nodes, gap_mode, t)) return rc;
    ParsRun run{c, b, t, gap_mode};
    if (int rc = run.start(parent, c->L, nullptr, true, false)) return rc;
    if (int rc = run.chunks(c->L, false, true, false, nullptr, 0, [&](int64_t j0, int64_t count) {
            LDW_HIP(hipMemcpyAsync(score_out + j0, b.score.p, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
            LDW_HIP(hipMemcpyAsync(min_out + j0, b.minch.p, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
            return (int)LDW_OK;
        }))
        return rc;
    LDW_HIP(hipStreamSynchronize(c->stream));
    return run.finish();
}

int states_run(ldw_ctx *c, const int32_t *parent, const int32_t *tip_seq, int64_t nodes, int32_t gap_mode, const int32_t *snp_idx, int64_t k, uint8_t *out,
               ParsBufs &b) {
    const char *who = "ldw_tree_states";
    LDW_REQUIRE(ldw::have_alignment(c), LDW_ERR_STATE, "%s: no alignment resident: set the alignment first", who);
    LDW_REQUIRE(k >= 1 && snp_idx, LDW_ERR_ARG, "%s: %lld SNPs (at least 1, and a list of them)", who, (long long)k);
    LDW_REQUIRE(out, LDW_ERR_ARG, "%s: output is null", who);
    LDW_REQUIRE(k < (1ll << 31), LDW_ERR_ARG, "%s: too many SNPs", who);
    ParsTree t;
    if (int rc = pars_check_tree(c, who, parent, tip_seq, nodes, gap_mode, t)) return rc;
    if (int rc = pars_check_snps(c, who, "snp_idx", snp_idx, k)) return rc;
    const ldw::DistinctSlots ds(snp_idx, k, nullptr, 0);
    const int64_t D = (int64_t)ds.d.size();
    ParsRun run{c, b, t, gap_mode};
    if (int rc = run.start(parent, D, ds.d.data(), false, true)) return rc;
    if (int rc = b.state.reserve((size_t)run.C * (size_t)nodes)) return rc;
    std::vector<uint8_t> rows((size_t)run.C * (size_t)nodes);
    if (int rc = run.chunks(D, true, false, true, nullptr, 0, [&](int64_t j0, int64_t count) {
            hipLaunchKernelGGL(k_pars_emit, dim3((unsigned)((nodes + 63) / 64), (unsigned)((count + 63) / 64)), dim3(256), 0, c->stream, b.sets.as<uint8_t>(),
                               run.Cpad, nodes, count, b.state.as<uint8_t>());
            LDW_HIP(hipGetLastError());
            LDW_HIP(hipMemcpyAsync(rows.data(), b.state.p, (size_t)count * (size_t)nodes, hipMemcpyDeviceToHost, c->stream));
            LDW_HIP(hipStreamSynchronize(c->stream));
            for (int64_t i = 0; i < k; ++i) {   // a SNP listed twice gets its row twice
                const int64_t s = ds.slot(snp_idx[i]);
                if (s >= j0 && s < j0 + count) memcpy(out + i * nodes, rows.data() + (s - j0) * nodes, (size_t)nodes);
            }
            return (int)LDW_OK;
        }))
        return rc;
    LDW_HIP(hipStreamSynchronize(c->stream));
    return run.finish();
}

int cochanges_run(ldw_ctx *c, const int32_t *parent, const int32_t *tip_seq, int64_t nodes, int32_t gap_mode, const int32_t *pair_a, const int32_t *pair_b,
                  int64_t K, int32_t *ca_out, int32_t *cb_out, int32_t *co_out, ParsBufs &b) {
    const char *who = "ldw_tree_cochanges";
    LDW_REQUIRE(ldw::have_alignment(c), LDW_ERR_STATE, "%s: no alignment resident: set the alignment first", who);
    LDW_REQUIRE(K >= 1 && pair_a && pair_b, LDW_ERR_ARG, "%s: %lld pairs (at least 1, and both lists of them)", who, (long long)K);
    LDW_REQUIRE(ca_out && cb_out && co_out, LDW_ERR_ARG, "%s: output is null", who);
    LDW_REQUIRE(K < (1ll << 30), LDW_ERR_ARG, "%s: too many pairs", who);
    ParsTree t;
    if (int rc = pars_check_tree(c, who, parent, tip_seq, nodes, gap_mode, t)) return rc;
    if (int rc = pars_check_snps(c, who, "pair_a", pair_a, K)) return rc;
    if (int rc = pars_check_snps(c, who, "pair_b", pair_b, K)) return rc;
    const ldw::DistinctSlots ds(pair_a, K, pair_b, K);
    const int64_t D = (int64_t)ds.d.size(), words = (nodes + 31) / 32;
    std::vector<int32_t> sa((size_t)K), sb((size_t)K);
    for (int64_t i = 0; i < K; ++i) sa[(size_t)i] = ds.slot(pair_a[i]), sb[(size_t)i] = ds.slot(pair_b[i]);
    ParsRun run{c, b, t, gap_mode};
    int rc = LDW_OK;
    if ((rc = run.start(parent, D, ds.d.data(), false, true)) || (rc = b.bits.reserve((size_t)words * (size_t)D * 4)) || (rc = ldw::upload(c, b.slot_a, sa.data(), sa.size())) ||
        (rc = ldw::upload(c, b.slot_b, sb.data(), sb.size())) || (rc = b.ca.reserve((size_t)K * 4)) || (rc = b.cb.reserve((size_t)K * 4)) ||
        (rc = b.co.reserve((size_t)K * 4)))
        return rc;
    if ((rc = run.chunks(D, true, false, true, b.bits.as<uint32_t>(), D, [](int64_t, int64_t) { return (int)LDW_OK; }))) return rc;
    // (the last event of the chunks stands in front of the pairs: their time is what finish() adds below)
    hipLaunchKernelGGL(k_pars_pairs, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, c->stream, b.bits.as<uint32_t>(), D, words, b.slot_a.as<int32_t>(),
                       b.slot_b.as<int32_t>(), K, b.ca.as<int32_t>(), b.cb.as<int32_t>(), b.co.as<int32_t>());
    LDW_HIP(hipGetLastError());
    LDW_HIP(hipEventRecord(c->ev[0], c->stream));
    LDW_HIP(hipMemcpyAsync(ca_out, b.ca.p, (size_t)K * 4, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemcpyAsync(cb_out, b.cb.p, (size_t)K * 4, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemcpyAsync(co_out, b.co.p, (size_t)K * 4, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    if ((rc = run.finish())) return rc;
    float pairs_ms = 0;
    LDW_HIP(hipEventElapsedTime(&pairs_ms, run.laps.ev.back(), c->ev[0]));
    c->last_ms[2] += pairs_ms, c->last_ms[3] += pairs_ms;
    return LDW_OK;
}

}  // namespace

extern "C" int ldw_tree_parsimony(ldw_ctx *c, const int32_t *parent, const int32_t *tip_seq, int64_t nodes, int32_t gap_mode, int32_t *score_out,
                                  int32_t *min_changes_out) {
    return ldw::scoped_call<ParsBufs>(c, [&](ParsBufs &b) { return parsimony_run(c, parent, tip_seq, nodes, gap_mode, score_out, min_changes_out, b); });
}

extern "C" int ldw_tree_states(ldw_ctx *c, const int32_t *parent, const int32_t *tip_seq, int64_t nodes, int32_t gap_mode, const int32_t *snp_idx, int64_t k,
                               uint8_t *node_state_out) {
    return ldw::scoped_call<ParsBufs>(c, [&](ParsBufs &b) { return states_run(c, parent, tip_seq, nodes, gap_mode, snp_idx, k, node_state_out, b); });
}

extern "C" int ldw_tree_cochanges(ldw_ctx *c, const int32_t *parent, const int32_t *tip_seq, int64_t nodes, int32_t gap_mode, const int32_t *pair_a,
                                  const int32_t *pair_b, int64_t K, int32_t *changes_a_out, int32_t *changes_b_out, int32_t *co_out) {
    return ldw::scoped_call<ParsBufs>(c, [&](ParsBufs &b) { return cochanges_run(c, parent, tip_seq, nodes, gap_mode, pair_a, pair_b, K, changes_a_out, changes_b_out, co_out, b); });
}
