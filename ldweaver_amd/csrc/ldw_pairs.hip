// Exact evaluation of the long-range candidates that the approximate screen lists pair by pair: see ldw_pairs.h.
//   k_pair_sums_q     exact joint sums by class-wise popcounts, a quarter-wave per pair (the default)
//   k_pair_sums       the same, a wave per pair; segment tables in LDS or in global memory
//   k_pair_sums_bits  the same sums by a walk over the set bits (weightings with many classes)
//   k_pair_mi         the sums -> fp64 MI -> emission
//   launch_pair_sums (choose_pair_form, ldw_pairs.h) / launch_pairs_exact
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "ldw_pairs.h"
#include "ldw_dev.h"

using namespace ldw;

namespace ldw {

// ------------------------------------------------------------------------------------------------
// The long-range candidates listed pair by pair (units without a short-range pair), in two kernels:
//   k_pair_sums_q<CA, CB>  a QUARTER-WAVE per pair (the 16 lanes of a DPP row), four pairs per wave, persistent waves: the default where
//                        the segment tables fit LDS (its own comment below; r08).  The same sums as:
//   k_pair_sums<CA, CB>  one WAVE per pair, lane = 32-bit word of the bit rows (coalesced 256-B reads of the pair's CA + CB rows
//                        from the row-major bit matrix).  sum_s V_s x_s y_s = sum_words sum_segments V_class popcount(x & y & mask):
//                        every lane multiplies the popcounts of ITS words by the class weight at once (one 64-bit multiply-add
//                        per segment) and a wave reduction adds the lanes up: no per-class flush, no serial walk over the row.
//                        The CA * CB exact sums of pair i of list `sub` go to sums[(sub * cap + i) * 16 + j * 4 + i].
//                        Runs where the tables stay in global memory, and under LDW_PAIR_WAVE=1 (the reference of the tests).
//   k_pair_mi<NA, NB>    one LANE per pair: the sums -> fp64 MI -> emission (candidate list + histogram).
// One pair in a few thousand gets here.
// ------------------------------------------------------------------------------------------------

// What the sum kernels share.
// Indicator row i of a SNP whose rows start at bit row r0 and number n (a PairEnt's ra / rb: r0 | n << 29), as words of W; an absent row is the row of zeros
template <class W>
__device__ __forceinline__ const W *pair_row(const PairArgs &P, int r0, int n, int i) {
    return reinterpret_cast<const W *>(P.Mbits + (int64_t)(i < n ? r0 + i : P.zero_row) * P.KW);
}
template <class W>
__device__ __forceinline__ const W *pair_row(const PairArgs &P, uint32_t r, int i) {
    return pair_row<W>(P, (int)(r & 0x1FFFFFFFu), (int)(r >> 29), i);
}
// one word pair against one segment: the weighted count of the positions of the segment that both rows hold
__device__ __forceinline__ int64_t pop_term(uint32_t f, uint32_t t, uint32_t mask, int64_t V) { return (int64_t)((uint64_t)__popc(f & t & mask) * (uint64_t)V); }

// CA x CB = 4 x 4 is the list of the pairs with a SNP of three or four indicator rows: nearly all of them 3 x 1 or 3 x 2, so the products with the
// absent rows (na, nb are wave-uniform: scalar branches) are skipped — r03 ran all sixteen against rows of zeros (k_pair_sums<true>: 1.0 ms per C4 pass)
template <int CA, int CB>
__device__ __forceinline__ void pair_sums_body(const PairArgs &P, int path, const int32_t *s_wbeg, const PopSeg *s_segs) {
    constexpr bool GENB = CA == 4 && CB == 4;
    const EpiArgs &A = P.A;
    const int sub = path * PAIR_SHARDS + (int)blockIdx.y;
    unsigned int n = A.pl_n[sub];
    n = n > A.pl_cap ? A.pl_cap : n;
    const int lane = threadIdx.x & 63;
    const PairEnt *list = A.pl_pairs + (int64_t)sub * A.pl_cap;
    // the segments of THIS lane's first words are the same for every pair: keep two per word in registers (a word holds more
    // than two only where several tiny weight classes meet: those go through the table)
    constexpr int KW = 3, KS = 2;
    uint32_t smask[KW][KS];
    int64_t sV[KW][KS];
    bool more[KW];
#pragma unroll
    for (int k = 0; k < KW; ++k) {
        const int w = lane + 64 * k;
        int s0 = 0, s1 = 0;
        if (w < P.nwords) {
            s0 = s_wbeg[w] & 0x7FFFFFFF;
            s1 = s_wbeg[w + 1] & 0x7FFFFFFF;
        }
        more[k] = s1 - s0 > KS;
#pragma unroll
        for (int q = 0; q < KS; ++q) {
            const bool on = s0 + q < s1 && !more[k];
            smask[k][q] = on ? s_segs[s0 + q].mask : 0u;
            sV[k][q] = on ? s_segs[s0 + q].V : 0;
        }
    }
    for (unsigned int idx = blockIdx.x * 4u + (threadIdx.x >> 6); idx < n; idx += gridDim.x * 4u) {
        const PairEnt e = list[idx];
        const uint32_t era = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.ra), erb = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.rb);
        const int r0a = (int)(era & 0x1FFFFFFFu), na = (int)(era >> 29), r0b = (int)(erb & 0x1FFFFFFFu), nb = (int)(erb >> 29);
        const uint32_t *fr[CA], *tr[CB];
#pragma unroll
        for (int i = 0; i < CA; ++i) fr[i] = pair_row<uint32_t>(P, r0a, na, i);
#pragma unroll
        for (int j = 0; j < CB; ++j) tr[j] = pair_row<uint32_t>(P, r0b, nb, j);
        int64_t s[CB][CA];
#pragma unroll
        for (int j = 0; j < CB; ++j)
#pragma unroll
            for (int i = 0; i < CA; ++i) s[j][i] = 0;
        // the first KW * 64 words: all loads of the pair are issued at once, the segments come from registers
        uint32_t f[KW][CA], tt[KW][CB];
#pragma unroll
        for (int k = 0; k < KW; ++k) {
            const int w = lane + 64 * k;
            const bool in = w < P.nwords;
#pragma unroll
            for (int i = 0; i < CA; ++i) f[k][i] = (in && (!GENB || i < na)) ? fr[i][w] : 0u;
#pragma unroll
            for (int j = 0; j < CB; ++j) tt[k][j] = (in && (!GENB || j < nb)) ? tr[j][w] : 0u;
        }
#pragma unroll
        for (int k = 0; k < KW; ++k) {
            if (more[k]) {
                const int w = lane + 64 * k;
                const int s0 = s_wbeg[w] & 0x7FFFFFFF, s1 = s_wbeg[w + 1] & 0x7FFFFFFF;
                for (int sg = s0; sg < s1; ++sg) {
                    const PopSeg seg = s_segs[sg];
#pragma unroll
                    for (int j = 0; j < CB; ++j)
#pragma unroll
                        for (int i = 0; i < CA; ++i)
                            if (!GENB || (i < na && j < nb)) s[j][i] += pop_term(f[k][i], tt[k][j], seg.mask, seg.V);
                }
            } else {
#pragma unroll
                for (int q2 = 0; q2 < KS; ++q2)
#pragma unroll
                    for (int j = 0; j < CB; ++j)
#pragma unroll
                        for (int i = 0; i < CA; ++i)
                            if (!GENB || (i < na && j < nb)) s[j][i] += pop_term(f[k][i], tt[k][j], smask[k][q2], sV[k][q2]);
            }
        }
        for (int w = lane + 64 * KW; w < P.nwords; w += 64) {   // longer rows (more than 6144 sequences): the rest through the table
            uint32_t f2[CA], t2[CB];
#pragma unroll
            for (int i = 0; i < CA; ++i) f2[i] = (!GENB || i < na) ? fr[i][w] : 0u;
#pragma unroll
            for (int j = 0; j < CB; ++j) t2[j] = (!GENB || j < nb) ? tr[j][w] : 0u;
            const int s0 = s_wbeg[w] & 0x7FFFFFFF, s1 = s_wbeg[w + 1] & 0x7FFFFFFF;
            for (int sg = s0; sg < s1; ++sg) {
                const PopSeg seg = s_segs[sg];
#pragma unroll
                for (int j = 0; j < CB; ++j)
#pragma unroll
                    for (int i = 0; i < CA; ++i)
                        if (!GENB || (i < na && j < nb)) s[j][i] += pop_term(f2[i], t2[j], seg.mask, seg.V);
            }
        }
#pragma unroll
        for (int j = 0; j < CB; ++j)
#pragma unroll
            for (int i = 0; i < CA; ++i) {
                int64_t v = s[j][i];
                if (!GENB || (i < na && j < nb)) {
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
                }
                if (lane == 0) P.sums[((int64_t)sub * A.pl_cap + idx) * 16 + j * 4 + i] = v;
            }
    }
}

// the four straight-line lists in one launch (blockIdx.z = path), the predicated one (16 sums per pair: many more registers)
// in another.  The segment tables are staged in LDS once per workgroup.
template <bool GEN>
__global__ __launch_bounds__(256) void k_pair_sums(PairArgs P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t pop_smem[];
    int32_t *s_wbeg = reinterpret_cast<int32_t *>(pop_smem);
    PopSeg *s_segs = reinterpret_cast<PopSeg *>(pop_smem + pop_seg_lds_bytes(P.nwords, 0));
    const int path = GEN ? 4 : (int)blockIdx.z;
    if (blockIdx.x * 4u >= P.A.pl_n[path * PAIR_SHARDS + (int)blockIdx.y]) return;   // nothing for this workgroup
    if (P.seg_in_lds) {
        for (int i = threadIdx.x; i < P.nwords + 1; i += 256) s_wbeg[i] = P.wbeg[i];
        for (int i = threadIdx.x; i < P.nseg; i += 256) s_segs[i] = P.segs[i];
        __syncthreads();
    } else {   // r04: thousands of weight classes (N distinct weights): the tables stay in global memory (L2-resident: every wave reads the same records)
        s_wbeg = const_cast<int32_t *>(P.wbeg);
        s_segs = const_cast<PopSeg *>(P.segs);
    }
    if constexpr (GEN) {
        pair_sums_body<4, 4>(P, 4, s_wbeg, s_segs);
    } else {
        switch (path) {
            case 0: pair_sums_body<1, 1>(P, 0, s_wbeg, s_segs); break;
            case 1: pair_sums_body<2, 1>(P, 1, s_wbeg, s_segs); break;
            case 2: pair_sums_body<1, 2>(P, 2, s_wbeg, s_segs); break;
            default: pair_sums_body<2, 2>(P, 3, s_wbeg, s_segs); break;
        }
    }
}

// r08: the same class-wise sums with a QUARTER-WAVE per pair and persistent waves (the default where the segment tables fit LDS; LDW_PAIR_WAVE=1
// launches the kernels above instead).  The 16 lanes of a DPP row own one pair, a wave works on four pairs at once.  Lane l of a row holds the words
// 32 k + 2 l, 32 k + 2 l + 1 of every row of its pair (one dwordx2 per row and step: a row of lanes reads 128 contiguous bytes), words past nwords
// read as zero.  The segments of those words are the same for every pair and stay in registers for PQ_KQ steps (160 words: 5 120 sequences), two per
// word; a word with more goes through the table in LDS, and so do the words of longer rows.  A workgroup stages the tables once, takes its one
// barrier, and its waves then walk the eight shards of their path as one index space (a prefix over the clamped counts) in strides of the whole
// grid, so a short shard idles nobody.  The loads of a wave's next four pairs (whose list entries were asked for one turn earlier still) are issued
// before the arithmetic of the current four.  The sixteen partial sums of a row are added with four DPP steps (two quad_perm, row_half_mirror,
// row_mirror), carry included; lane 0 of the row stores them where k_pair_mi reads them.  Same int64 terms in another order: the same sums.
constexpr int PQ_KQ = 5, PQ_KS = 2;
constexpr int PQ_WGS_PER_CU = 2;   // workgroups per CU and path (LDW_PAIR_GRID: A/B; profiles/r08_pair_sums_quarter.txt)

template <int CTRL>
__device__ __forceinline__ int64_t dpp_add64(int64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xF, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)((uint64_t)v >> 32), CTRL, 0xF, 0xF, false);
    return v + (int64_t)(((uint64_t)hi << 32) | (uint64_t)lo);
}
// the sum over the 16 lanes of a DPP row, in every lane of it (all 64 lanes active)
__device__ __forceinline__ int64_t row16_sum(int64_t v) {
    v = dpp_add64<0xB1>(v);    // quad_perm [1, 0, 3, 2]
    v = dpp_add64<0x4E>(v);    // quad_perm [2, 3, 0, 1]
    v = dpp_add64<0x141>(v);   // row_half_mirror
    v = dpp_add64<0x140>(v);   // row_mirror
    return v;
}

template <int CA, int CB, bool PREF>
__device__ __forceinline__ void pair_sums_q_body(const PairArgs &P, int path, const int32_t *s_wbeg, const PopSeg *s_segs) {
    constexpr bool GENB = CA == 4 && CB == 4;
    constexpr int KQ = PQ_KQ, KS = PQ_KS;
    const EpiArgs &A = P.A;
    const int lane = threadIdx.x & 63, l = lane & 15, grp = lane >> 4;
    // the eight shards of the path as one index space
    unsigned int pre[PAIR_SHARDS + 1];
    pre[0] = 0u;
#pragma unroll
    for (int s = 0; s < PAIR_SHARDS; ++s) {
        const unsigned int n = A.pl_n[path * PAIR_SHARDS + s];
        pre[s + 1] = pre[s] + (n > A.pl_cap ? A.pl_cap : n);
    }
    const unsigned int total = pre[PAIR_SHARDS];
    const unsigned int nwv = gridDim.x * 4u;
    unsigned int t = blockIdx.x * 4u + (threadIdx.x >> 6);   // four pairs 4 t .. 4 t + 3 per turn of a wave
    if (4u * t >= total) return;
    const PairEnt *lists = A.pl_pairs + (int64_t)path * PAIR_SHARDS * A.pl_cap;
    auto locate = [&](unsigned int p, int &shard, unsigned int &idx) {
        shard = 0;
        unsigned int base = 0u;
#pragma unroll
        for (int s = 1; s < PAIR_SHARDS; ++s)
            if (p >= pre[s]) shard = s, base = pre[s];
        idx = p - base;
    };
    // (ra, rb) of this row's pair of turn tt; (0, 0) — no rows — behind the end of the lists
    auto load_ent = [&](unsigned int tt) -> uint2 {
        const unsigned int p = 4u * tt + (unsigned int)grp;
        if (p >= total) return make_uint2(0u, 0u);
        int shard;
        unsigned int idx;
        locate(p, shard, idx);
        const PairEnt *e = lists + (int64_t)shard * A.pl_cap + idx;
        return make_uint2(e->ra, e->rb);
    };
    auto issue_rows = [&](uint2 e, uint2 (&f)[KQ][CA], uint2 (&tt)[KQ][CB]) {
        const int na = (int)(e.x >> 29), nb = (int)(e.y >> 29);
#pragma unroll
        for (int i = 0; i < CA; ++i) {
            const uint2 *fr = pair_row<uint2>(P, e.x, i);
#pragma unroll
            for (int k = 0; k < KQ; ++k) f[k][i] = (32 * k + 2 * l < P.nwords && (!GENB || i < na)) ? fr[16 * k + l] : make_uint2(0u, 0u);
        }
#pragma unroll
        for (int j = 0; j < CB; ++j) {
            const uint2 *tr = pair_row<uint2>(P, e.y, j);
#pragma unroll
            for (int k = 0; k < KQ; ++k) tt[k][j] = (32 * k + 2 * l < P.nwords && (!GENB || j < nb)) ? tr[16 * k + l] : make_uint2(0u, 0u);
        }
    };
    // the segments of THIS lane's words (the same in the four rows of the wave)
    uint32_t smask[KQ][2][KS];
    int64_t sV[KQ][2][KS];
    uint32_t more = 0u;
#pragma unroll
    for (int k = 0; k < KQ; ++k)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int w = 32 * k + 2 * l + h;
            int s0 = 0, s1 = 0;
            if (w < P.nwords) {
                s0 = s_wbeg[w] & 0x7FFFFFFF;
                s1 = s_wbeg[w + 1] & 0x7FFFFFFF;
            }
            const bool mr = s1 - s0 > KS;
            if (mr) more |= 1u << (2 * k + h);
#pragma unroll
            for (int q = 0; q < KS; ++q) {
                const bool on = s0 + q < s1 && !mr;
                smask[k][h][q] = on ? s_segs[s0 + q].mask : 0u;
                sV[k][h][q] = on ? s_segs[s0 + q].V : 0;
            }
        }
    uint2 e_cur = load_ent(t);
    uint2 f[KQ][CA], tt[KQ][CB];
    issue_rows(e_cur, f, tt);
    unsigned int tn = t + nwv;
    uint2 e_nx = load_ent(tn);
    for (;;) {
        const bool has_nx = 4u * tn < total;   // wave-uniform
        uint2 fn[KQ][CA], tnx[KQ][CB];
        uint2 e_nx2 = make_uint2(0u, 0u);
        if (PREF && has_nx) {
            issue_rows(e_nx, fn, tnx);
            e_nx2 = load_ent(tn + nwv);
        }
        const int na = (int)(e_cur.x >> 29), nb = (int)(e_cur.y >> 29);
        // the predicated list: rows differ in (na, nb); an absent row was not loaded and adds zero, the loops stop at the wave's largest
        int namax = CA, nbmax = CB;
        if constexpr (GENB) {
            namax = 1 + (__ballot(na >= 2) != 0ull) + (__ballot(na >= 3) != 0ull) + (__ballot(na >= 4) != 0ull);
            nbmax = 1 + (__ballot(nb >= 2) != 0ull) + (__ballot(nb >= 3) != 0ull) + (__ballot(nb >= 4) != 0ull);
        }
        int64_t s[CB][CA];
#pragma unroll
        for (int j = 0; j < CB; ++j)
#pragma unroll
            for (int i = 0; i < CA; ++i) s[j][i] = 0;
#pragma unroll
        for (int k = 0; k < KQ; ++k) {
            if (32 * k >= P.nwords) break;   // (uniform)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                uint32_t fw[CA], tw[CB];
#pragma unroll
                for (int i = 0; i < CA; ++i) fw[i] = h ? f[k][i].y : f[k][i].x;
#pragma unroll
                for (int j = 0; j < CB; ++j) tw[j] = h ? tt[k][j].y : tt[k][j].x;
#pragma unroll
                for (int q = 0; q < KS; ++q)
#pragma unroll
                    for (int j = 0; j < CB; ++j)
#pragma unroll
                        for (int i = 0; i < CA; ++i)
                            if (!GENB || (i < namax && j < nbmax)) s[j][i] += pop_term(fw[i], tw[j], smask[k][h][q], sV[k][h][q]);
                if ((more >> (2 * k + h)) & 1u) {   // more than KS segments in this lane's word (its registers hold none of them)
                    const int w = 32 * k + 2 * l + h;
                    const int s0 = s_wbeg[w] & 0x7FFFFFFF, s1 = s_wbeg[w + 1] & 0x7FFFFFFF;
                    for (int sg = s0; sg < s1; ++sg) {
                        const PopSeg seg = s_segs[sg];
#pragma unroll
                        for (int j = 0; j < CB; ++j)
#pragma unroll
                            for (int i = 0; i < CA; ++i)
                                if (!GENB || (i < namax && j < nbmax)) s[j][i] += pop_term(fw[i], tw[j], seg.mask, seg.V);
                    }
                }
            }
        }
        if (32 * KQ < P.nwords) {   // longer rows: the rest through the table (absent rows: the row of zeros)
            const uint2 *fr[CA], *tr[CB];
#pragma unroll
            for (int i = 0; i < CA; ++i) fr[i] = pair_row<uint2>(P, e_cur.x, i);
#pragma unroll
            for (int j = 0; j < CB; ++j) tr[j] = pair_row<uint2>(P, e_cur.y, j);
            for (int w2 = 16 * KQ + l; 2 * w2 < P.nwords; w2 += 16) {
                uint2 f2[CA], t2[CB];
#pragma unroll
                for (int i = 0; i < CA; ++i) f2[i] = fr[i][w2];
#pragma unroll
                for (int j = 0; j < CB; ++j) t2[j] = tr[j][w2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int w = 2 * w2 + h;
                    const int s0 = s_wbeg[w] & 0x7FFFFFFF, s1 = s_wbeg[w + 1] & 0x7FFFFFFF;
                    for (int sg = s0; sg < s1; ++sg) {
                        const PopSeg seg = s_segs[sg];
#pragma unroll
                        for (int j = 0; j < CB; ++j)
#pragma unroll
                            for (int i = 0; i < CA; ++i)
                                if (!GENB || (i < namax && j < nbmax))
                                    s[j][i] += pop_term((h ? f2[i].y : f2[i].x), (h ? t2[j].y : t2[j].x), seg.mask, seg.V);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < CB; ++j)
#pragma unroll
            for (int i = 0; i < CA; ++i)
                if (!GENB || (i < namax && j < nbmax)) s[j][i] = row16_sum(s[j][i]);
        const unsigned int p = 4u * t + (unsigned int)grp;
        if (l == 0 && p < total) {
            int shard;
            unsigned int idx;
            locate(p, shard, idx);
            int64_t *o = P.sums + ((int64_t)(path * PAIR_SHARDS + shard) * A.pl_cap + idx) * 16;
#pragma unroll
            for (int j = 0; j < CB; ++j)
#pragma unroll
                for (int i = 0; i < CA; ++i) o[j * 4 + i] = s[j][i];
        }
        if (!has_nx) break;
        t = tn;
        tn += nwv;
        e_cur = e_nx;
        if constexpr (PREF) {
#pragma unroll
            for (int k = 0; k < KQ; ++k) {
#pragma unroll
                for (int i = 0; i < CA; ++i) f[k][i] = fn[k][i];
#pragma unroll
                for (int j = 0; j < CB; ++j) tt[k][j] = tnx[k][j];
            }
            e_nx = e_nx2;
        } else {
            issue_rows(e_cur, f, tt);
            e_nx = load_ent(tn);
        }
    }
}

template <bool GEN>
__global__ __launch_bounds__(256) void k_pair_sums_q(PairArgs P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t pop_smem[];
    int32_t *s_wbeg = reinterpret_cast<int32_t *>(pop_smem);
    PopSeg *s_segs = reinterpret_cast<PopSeg *>(pop_smem + pop_seg_lds_bytes(P.nwords, 0));
    const int path = GEN ? 4 : (int)blockIdx.z;
    unsigned int total = 0u;
    for (int s = 0; s < PAIR_SHARDS; ++s) {
        const unsigned int n = P.A.pl_n[path * PAIR_SHARDS + s];
        total += n > P.A.pl_cap ? P.A.pl_cap : n;
    }
    if (blockIdx.x * 16u >= total) return;   // nothing for this workgroup
    for (int i = threadIdx.x; i < P.nwords + 1; i += 256) s_wbeg[i] = P.wbeg[i];
    for (int i = threadIdx.x; i < P.nseg; i += 256) s_segs[i] = P.segs[i];
    __syncthreads();
    if constexpr (GEN) {
        pair_sums_q_body<4, 4, false>(P, 4, s_wbeg, s_segs);
    } else {
        switch (path) {
            case 0: pair_sums_q_body<1, 1, true>(P, 0, s_wbeg, s_segs); break;
            case 1: pair_sums_q_body<2, 1, true>(P, 1, s_wbeg, s_segs); break;
            case 2: pair_sums_q_body<1, 2, true>(P, 2, s_wbeg, s_segs); break;
            default: pair_sums_q_body<2, 2, true>(P, 3, s_wbeg, s_segs); break;
        }
    }
}

// r05: the same exact sums for weightings with MANY classes (every sequence its own weight: hdw = 1 / (k + 1) with all k distinct, the bench's
// adversarial "distinct weights" case).  The class-wise form above then walks one segment per POSITION — 32 records per word, read from global
// memory because 5 000 records do not fit LDS: 1.37 ms per launch, 38 ms of an 85 ms pass, bound by the L2.  Here a lane walks the SET BITS of
// its words instead (two SNPs' minor states co-occur in a few sequences per word) and adds the weight of each position from a table in LDS,
// laid out [bit][word] so that the lanes of a wave — different words, any bit — never share a bank (stride a multiple of 32 words).
// Same integers (a sum of the same int64 terms in another order), so the tables downstream are bit-identical.
template <int CA, int CB>
__device__ __forceinline__ void pair_sums_bits_body(const PairArgs &P, int path, const int64_t *sVT, int stride) {
    constexpr bool GENB = CA == 4 && CB == 4;
    const EpiArgs &A = P.A;
    const int sub = path * PAIR_SHARDS + (int)blockIdx.y;
    unsigned int n = A.pl_n[sub];
    n = n > A.pl_cap ? A.pl_cap : n;
    const int lane = threadIdx.x & 63;
    const PairEnt *list = A.pl_pairs + (int64_t)sub * A.pl_cap;
    for (unsigned int idx = blockIdx.x * 4u + (threadIdx.x >> 6); idx < n; idx += gridDim.x * 4u) {
        const PairEnt e = list[idx];
        const uint32_t era = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.ra), erb = (uint32_t)__builtin_amdgcn_readfirstlane((int)e.rb);
        const int r0a = (int)(era & 0x1FFFFFFFu), na = (int)(era >> 29), r0b = (int)(erb & 0x1FFFFFFFu), nb = (int)(erb >> 29);
        const uint32_t *fr[CA], *tr[CB];
#pragma unroll
        for (int i = 0; i < CA; ++i) fr[i] = pair_row<uint32_t>(P, r0a, na, i);
#pragma unroll
        for (int j = 0; j < CB; ++j) tr[j] = pair_row<uint32_t>(P, r0b, nb, j);
        int64_t s[CB][CA];
#pragma unroll
        for (int j = 0; j < CB; ++j)
#pragma unroll
            for (int i = 0; i < CA; ++i) s[j][i] = 0;
        for (int w = lane; w < P.nwords; w += 64) {
            uint32_t f[CA], t[CB], uf = 0u, ut = 0u;
#pragma unroll
            for (int i = 0; i < CA; ++i) {
                f[i] = (!GENB || i < na) ? fr[i][w] : 0u;
                uf |= f[i];
            }
#pragma unroll
            for (int j = 0; j < CB; ++j) {
                t[j] = (!GENB || j < nb) ? tr[j][w] : 0u;
                ut |= t[j];
            }
            uint32_t u = uf & ut;   // positions where SOME row of a and some row of b are set
            while (u) {
                const int b = __builtin_ctz(u);
                u &= u - 1u;
                const int64_t v = sVT[b * stride + w];
#pragma unroll
                for (int j = 0; j < CB; ++j)
#pragma unroll
                    for (int i = 0; i < CA; ++i)
                        if (CA * CB == 1 || (((f[i] & t[j]) >> b) & 1u)) s[j][i] += v;
            }
        }
#pragma unroll
        for (int j = 0; j < CB; ++j)
#pragma unroll
            for (int i = 0; i < CA; ++i) {
                int64_t v = s[j][i];
                if (!GENB || (i < na && j < nb)) {
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
                }
                if (lane == 0) P.sums[((int64_t)sub * A.pl_cap + idx) * 16 + j * 4 + i] = v;
            }
    }
}

template <bool GEN>
__global__ __launch_bounds__(256) void k_pair_sums_bits(PairArgs P, const int64_t *__restrict__ vpos, int stride) {
    extern __shared__ __attribute__((aligned(16))) uint8_t pop_smem[];
    int64_t *sVT = reinterpret_cast<int64_t *>(pop_smem);
    const int path = GEN ? 4 : (int)blockIdx.z;
    if (blockIdx.x * 4u >= P.A.pl_n[path * PAIR_SHARDS + (int)blockIdx.y]) return;   // nothing for this workgroup
    for (int i = threadIdx.x; i < 32 * stride; i += 256) {
        const int b = i / stride, w = i - b * stride;
        sVT[i] = w < P.nwords ? vpos[32 * w + b] : 0;
    }
    __syncthreads();
    if constexpr (GEN) {
        pair_sums_bits_body<4, 4>(P, 4, sVT, stride);
    } else {
        switch (path) {
            case 0: pair_sums_bits_body<1, 1>(P, 0, sVT, stride); break;
            case 1: pair_sums_bits_body<2, 1>(P, 1, sVT, stride); break;
            case 2: pair_sums_bits_body<1, 2>(P, 2, sVT, stride); break;
            default: pair_sums_bits_body<2, 2>(P, 3, sVT, stride); break;
        }
    }
}

// Emission of the listed pairs.  Nearly all of them ARE candidates (they sit in the few buckets just above the guess), so one
// returning atomic on the candidate counter plus one histogram atomic per pair made the kernel a queue at two or three
// addresses of the L2 (100 us for 7e4 pairs; 14 us with the atomics compiled out): a wave bumps the counter ONCE for all its
// candidates, and the bucket counts go through a workgroup-local window of PAIR_HWIN buckets in LDS, flushed at the end.
constexpr int PAIR_HWIN = 128;

template <int NA, int NB>   // NA = 0: any slot counts (predicated code)
__device__ __forceinline__ void pair_mi_body(const PairArgs &P, int path, unsigned int *s_hist) {
    constexpr bool GEN = NA == 0;
    const EpiArgs &A = P.A;
    const EmitArgs &E = A.E;
    const int sub = path * PAIR_SHARDS + (int)blockIdx.y;
    unsigned int n = A.pl_n[sub];
    n = n > A.pl_cap ? A.pl_cap : n;
    const bool square = A.nf == A.nt;
    const PairEnt *list = A.pl_pairs + (int64_t)sub * A.pl_cap;
    const int lane = (int)(threadIdx.x & 63);
    // wave-uniform trip count: every lane stays in the loop, so the ballots below see the whole wave
    for (unsigned int base = blockIdx.x * 256u + (threadIdx.x & ~63u); base < n; base += gridDim.x * 256u) {
        const unsigned int idx = base + (unsigned int)lane;
        bool valid = idx < n;
        uint32_t t = 0, q = 0;
        if (valid) {
            t = list[idx].t;
            q = list[idx].q;
        }
        const RowPack &RP = A.rowpack[t];
        valid = valid && RP.a_loc >= 0;
        bool cand = false;
        int bk = 0, seg = -1, a_loc = 0, b_loc = 0, sg = 0;
        double mi = 0.0;
        if (valid) {
            const RowSide R = RP.R;
            a_loc = RP.a_loc;
            const ColMeta M = A.colpack[q];
            b_loc = M.bl;
            sg = A.span ? M.ci.pad[0] : 0;   // a span: the reference block (segment) of the column; b_loc is local to it
            const int64_t *sp = P.sums + ((int64_t)sub * A.pl_cap + idx) * 16;
            if constexpr (GEN) {
                mi = pair_mi<4, 4>(A, R, M, a_loc, b_loc, square, gacc_plain(sp, 1, 4));
            } else {
                mi = pair_mi_full<NA, NB>(A, R, M, a_loc, b_loc, square, gacc_plain(sp, 1, 4));
            }
            seg = pair_seg(a_loc, b_loc, E.lower_only);
            if (seg >= 0 && E.any_sr && col_is_sr(M.ci, a_loc)) {
                emit_pair_spec(E, M.ci, a_loc, b_loc, R.sa, M.sb, mi, P.ghist);   // (a short-range pair is never listed; kept for exactness)
            } else if (seg >= 0 && E.do_lr && mi >= E.spec_lo) {
                bk = mi_bucket(mi);
                cand = bk >= E.spec_B;
            }
        }
        if (A.span) {
            // every reference block of the span keeps its own candidate list and histogram (the long-range filter is per block:
            // R/computePairwiseMI.R:352-358); the lanes of a wave hold columns of any segment (the to side is ordered by weight)
            for (int k = 0; k < A.span; ++k) {
                const bool mine = cand && sg == k;
                const unsigned long long mk = __ballot(mine);
                if (mk == 0ull) continue;
                const int leader = __builtin_ctzll(mk);
                unsigned long long pos = 0;
                if (lane == leader) pos = atomicAdd(A.sseg[k].n_cand, (unsigned long long)__popcll(mk));
                pos = __shfl(pos, leader);
                if (mine) {
                    pos += (unsigned long long)__popcll(mk & ((1ull << lane) - 1ull));
                    A.sseg[k].ckey[pos] = f64_key(mi);
                    A.sseg[k].cval[pos] = ((uint64_t)seg << 62) | ((uint64_t)a_loc + (uint64_t)b_loc * (uint64_t)E.nf);
                    const int w = bk - (E.spec_B > 0 ? E.spec_B : 0);
                    if (w < PAIR_HWIN) atomicAdd(&s_hist[k * PAIR_HWIN + w], 1u);
                    else atomicAdd(&A.sseg[k].ghist[bk], 1ull);
                }
            }
            continue;
        }
        const unsigned long long mk = __ballot(cand);
        if (mk == 0ull) continue;
        const int leader = __builtin_ctzll(mk);
        unsigned long long pos = 0;
        if (lane == leader) pos = atomicAdd(E.n_cand, (unsigned long long)__popcll(mk));
        pos = __shfl(pos, leader);
        if (cand) {
            pos += (unsigned long long)__popcll(mk & ((1ull << lane) - 1ull));
            E.ckey[pos] = f64_key(mi);
            E.cval[pos] = ((uint64_t)seg << 62) | ((uint64_t)a_loc + (uint64_t)b_loc * (uint64_t)E.nf);
            const int w = bk - (E.spec_B > 0 ? E.spec_B : 0);
            if (w < PAIR_HWIN) atomicAdd(&s_hist[w], 1u);
            else atomicAdd(&P.ghist[bk], 1ull);
        }
    }
}

__global__ __launch_bounds__(256) void k_pair_mi(PairArgs P) {
    __shared__ unsigned int s_hist[LDW_SPAN_MAX * PAIR_HWIN];   // one bucket window per segment of a span (segment 0: an ordinary block)
    for (int i = threadIdx.x; i < LDW_SPAN_MAX * PAIR_HWIN; i += 256) s_hist[i] = 0u;
    __syncthreads();
    switch (blockIdx.z) {
        case 0: pair_mi_body<1, 1>(P, 0, s_hist); break;
        case 1: pair_mi_body<2, 1>(P, 1, s_hist); break;
        case 2: pair_mi_body<1, 2>(P, 2, s_hist); break;
        case 3: pair_mi_body<2, 2>(P, 3, s_hist); break;
        default: pair_mi_body<0, 0>(P, 4, s_hist); break;
    }
    __syncthreads();
    const int hb0 = P.A.E.spec_B > 0 ? P.A.E.spec_B : 0;
    if (P.A.span) {
        for (int i = threadIdx.x; i < P.A.span * PAIR_HWIN; i += 256) {
            const int k = i / PAIR_HWIN, w = i - k * PAIR_HWIN;
            if (s_hist[i] != 0u && hb0 + w < NBINS) atomicAdd(&P.A.sseg[k].ghist[hb0 + w], (unsigned long long)s_hist[i]);
        }
        return;
    }
    if (threadIdx.x < PAIR_HWIN && s_hist[threadIdx.x] != 0u && hb0 + (int)threadIdx.x < NBINS)
        atomicAdd(&P.ghist[hb0 + threadIdx.x], (unsigned long long)s_hist[threadIdx.x]);
}

static PairArgs make_pair_args(ldw_ctx *c, const EpiArgs &A, unsigned long long *ghist, int64_t *sums) {
    PairArgs P;
    memset(&P, 0, sizeof(P));
    P.Mbits = c->rows.Mbits.as<uint64_t>();
    P.KW = c->KW;
    P.nwords = (int)(c->KW * 2);
    P.nseg = c->apx.n_pop_segs;
    P.segs = c->apx.pop_segs.as<PopSeg>();
    P.wbeg = c->apx.pop_wbeg.as<int32_t>();
    P.row0 = c->rows.row0.as<int32_t>();
    P.zero_row = (int32_t)c->rows.R;
    P.sums = sums;
    P.A = A;
    P.ghist = ghist;
    return P;
}

// The exact sums of every list: takes the form that choose_pair_form gives for the weighting (PAIR_FORM_AUTO) or for the caller's request
// (ldw_debug_pair_sums; its error before anything is launched) and launches its two kernels.  grid_wgs 0: the product's grid; else gridDim.x of both launches.
int launch_pair_sums(ldw_ctx *c, const EpiArgs &A, int64_t *sums, hipStream_t st, int form, int grid_wgs, PairSumsRan *ran) {
    PairArgs P = make_pair_args(c, A, nullptr, sums);
    const char *wv = getenv("LDW_PAIR_WAVE");   // (both read per call: A/B, and the tests run every form)
    const PairFormChoice ch = choose_pair_form(P.nwords, P.nseg, c->apx.pop_vpos.p != nullptr, wv && atoi(wv) != 0, getenv("LDW_NO_PAIR_BITS") != nullptr, form);
    LDW_REQUIRE(ch.rc == LDW_OK, ch.rc, "%s", ch.msg);
    P.seg_in_lds = ch.seg_in_lds;
    static const unsigned grid_env = [] { const char *e = getenv("LDW_PAIR_GRID"); return e ? (unsigned)atoi(e) : 0u; }();   // (A/B)
    const unsigned gforce = grid_wgs > 0 ? (unsigned)grid_wgs : 0u;
    if (ch.form == PAIR_FORM_BITS) {
        if (ch.lds160 && !c->pair_bits_attr) {
            LDW_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_pair_sums_bits<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)PAIR_BITS_LDS_MAX));
            LDW_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_pair_sums_bits<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)PAIR_BITS_LDS_MAX));
            c->pair_bits_attr = true;
        }
        const unsigned gx = gforce ? gforce : 256u;
        const int stride = pair_bits_stride(P.nwords);
        hipLaunchKernelGGL(k_pair_sums_bits<false>, dim3(gx, PAIR_SHARDS, 4), dim3(256), ch.lds, st, P, c->apx.pop_vpos.as<int64_t>(), stride);
        hipLaunchKernelGGL(k_pair_sums_bits<true>, dim3(gx, PAIR_SHARDS, 1), dim3(256), ch.lds, st, P, c->apx.pop_vpos.as<int64_t>(), stride);
    } else if (ch.form == PAIR_FORM_QUARTER) {
        // r08: a quarter-wave per pair, persistent waves: LDW_PAIR_GRID (or PQ_WGS_PER_CU) workgroups per CU for every path; those beyond a
        // path's pairs leave before staging.  LDW_PAIR_GRID_WGS (read per call: the tests force turns on small lists) sets the whole grid of a path.
        unsigned gx = (grid_env ? grid_env : (unsigned)PQ_WGS_PER_CU) * (unsigned)std::max(c->n_cu, 1);
        if (const char *e = getenv("LDW_PAIR_GRID_WGS")) {
            const int k = atoi(e);
            if (k > 0 && k <= 65536) gx = (unsigned)k;
        }
        if (gforce) gx = gforce;
        hipLaunchKernelGGL(k_pair_sums_q<false>, dim3(gx, 1, 4), dim3(256), ch.lds, st, P);
        hipLaunchKernelGGL(k_pair_sums_q<true>, dim3(gx, 1, 1), dim3(256), ch.lds, st, P);
    } else {
        // (grid: r06 — 512 / 1024 workgroups per list instead of 256: 67 -> 61 and 34 -> 23 us per launch; 128 / 64 / 32: 96 / 150 / 236 us.  A 1-D grid whose
        // waves share the pairs of all lists evenly was built too: no better (64 / 42 us) — the long launches are not a matter of balance.)
        hipLaunchKernelGGL(k_pair_sums<false>, dim3(gforce ? gforce : grid_env ? grid_env : 512u, PAIR_SHARDS, 4), dim3(256), ch.lds, st, P);
        hipLaunchKernelGGL(k_pair_sums<true>, dim3(gforce ? gforce : grid_env ? grid_env : 1024u, PAIR_SHARDS, 1), dim3(256), ch.lds, st, P);
    }
    ran->form = ch.form;
    ran->lds160 = ch.lds160;
    return LDW_OK;
}

int launch_pairs_exact(ldw_ctx *c, const EpiArgs &A, unsigned long long *ghist, int64_t *sums, hipStream_t st) {
    // the exact sums of every list (a quarter-wave per pair, or one of the wave-per-pair forms), then one lane per pair for the fp64 value
    PairSumsRan ran;
    if (int rc = launch_pair_sums(c, A, sums, st, PAIR_FORM_AUTO, 0, &ran)) return rc;
    switch (ran.form) {
        case PAIR_FORM_BITS: c->cnt.form_launches[ran.lds160 ? 1 : 0] += 2; break;
        case PAIR_FORM_QUARTER: c->cnt.form_launches[2] += 2, c->cnt.pair_kernel_launches[0] += 2; break;
        case PAIR_FORM_WAVE_LDS: c->cnt.form_launches[2] += 2, c->cnt.pair_kernel_launches[1] += 2; break;
        default: c->cnt.form_launches[3] += 2, c->cnt.pair_kernel_launches[1] += 2; break;
    }
    const PairArgs P = make_pair_args(c, A, ghist, sums);
    hipLaunchKernelGGL(k_pair_mi, dim3(64, PAIR_SHARDS, PAIR_PATHS), dim3(256), 0, st, P);
    LDW_HIP(hipGetLastError());
    return LDW_OK;
}

void warm_pairs() {   // ldw_ctx_create's side thread: load this translation unit's code object ahead of its first launch
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_pair_mi));
    (void)hipGetLastError();
}

}  // namespace ldw
