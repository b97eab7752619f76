// Approximate-GEMM path of the speculative blocks: see ldw_apx.h for the formulation.
//   prepare_apx_weights  host: dual digits a, b and block exponents of the weights; uploads the popcount segment tables (build_pop_segs, ldw_pairs.h)
//   k_pack_panel         per block side: bit rows of the row list, transposed to [macro step][row][2 words]
//   k_apx_live_tiles     which wave tiles the GEMM has to compute at all
//   gemm_apx_kernel      one int8 MFMA pass, both operands masked digits -> int32 approximate joint sums (screen input)
// (The exact sums of the pairs the screen then lists: ldw_pairs.hip.)
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "ldw_apx.h"
#include "ldw_pairs.h"
#include "ldw_dev.h"

using namespace ldw;

namespace ldw {

// ------------------------------------------------------------------------------------------------
// host: weights -> (a, b, e)
// ------------------------------------------------------------------------------------------------
namespace {
constexpr int64_t APX_PROD_CAP = 12000;
struct ProdTable {
    std::vector<int32_t> val;
    std::vector<uint8_t> a, b;
    ProdTable() {
        std::vector<std::pair<int32_t, std::pair<uint8_t, uint8_t>>> all;
        for (int x = 0; x <= 127; ++x)
            for (int y = x; y <= 127; ++y) all.push_back({x * y, {(uint8_t)x, (uint8_t)y}});
        std::sort(all.begin(), all.end());
        for (auto &e : all)
            if (val.empty() || val.back() != e.first) {
                val.push_back(e.first);
                a.push_back(e.second.first);
                b.push_back(e.second.second);
            }
    }
    // index of the product nearest to t (0 <= t <= 16129)
    size_t nearest(double t) const {
        size_t hi = std::lower_bound(val.begin(), val.end(), (int32_t)std::ceil(t)) - val.begin();
        if (hi >= val.size()) hi = val.size() - 1;
        size_t lo = hi > 0 ? hi - 1 : 0;
        return (t - (double)val[lo]) <= ((double)val[hi] - t) ? lo : hi;
    }
};
}  // namespace

int prepare_apx_weights(ldw_ctx *c) {
    static const ProdTable PT;
    const int64_t N = c->N, Npad = c->Npad;
    const int M2 = (int)(Npad / 128);
    c->apx.apx_ok = false;
    std::vector<int64_t> Vp((size_t)Npad, 0);
    for (int64_t p = 0; p < N; ++p) Vp[(size_t)p] = c->wts.h_vfixed[(size_t)c->wts.h_seq_perm[(size_t)p]];
    // block exponents, one per MFMA k-step of 32 consecutive positions (r03; r02 had one per macro step of 128, which put weights
    // 1/128 .. 1 of an alignment with N distinct weights under ONE exponent: delta 6e-3, path off): smallest non-decreasing e(k)
    // with ceil(Vmax(k) / 2^e) <= APX_PROD_CAP.  Products of two 7-bit digits are dense up to ~12000 (worst relative half-gap
    // 1.0e-3 over [6000, 12000], 1.2e-3 over [3000, 12000]) and sparse above (15750 -> 15875: 4e-3), so the largest weight of a
    // step is mapped below the sparse region
    const int S4 = 4 * M2;
    std::vector<int32_t> em((size_t)S4, 0), sh((size_t)S4, 0);
    std::vector<uint8_t> da((size_t)Npad, 0), db((size_t)Npad, 0);
    double delta = 0;
    int transitions = 0;
    // gran = 4: one exponent per macro step of 128 positions (the faster kernel variant); gran = 1: one per k-step.  The coarse form
    // is kept whenever it is tight enough (delta <= 1.5e-3: the screen's margin grows with delta)
    auto assign = [&](int gran) {
        std::fill(sh.begin(), sh.end(), 0);
        std::fill(da.begin(), da.end(), 0);
        std::fill(db.begin(), db.end(), 0);
        c->apx.h_vapx.assign((size_t)Npad, 0);
        int e_prev = 0;
        transitions = 0;
        for (int k0 = 0; k0 < S4; k0 += gran) {
            int64_t vmax = 0;
            for (int q = 0; q < 32 * gran; ++q) vmax = std::max(vmax, Vp[(size_t)k0 * 32 + q]);
            int e = e_prev;
            while (e < 62 && ((vmax + ((int64_t)1 << e) - 1) >> e) > APX_PROD_CAP) ++e;
            for (int k = k0; k < k0 + gran; ++k) em[(size_t)k] = e;
            if (k0 > 0 && e > e_prev) {
                sh[(size_t)k0] = std::min(e - e_prev, 31);
                ++transitions;
            }
            e_prev = e;
        }
        delta = 0;
        for (int64_t p = 0; p < N; ++p) {
            const int64_t V = Vp[(size_t)p];
            if (V <= 0) continue;
            const int e = em[(size_t)(p / 32)];
            const size_t k = PT.nearest(std::ldexp((double)V, -e));
            da[(size_t)p] = PT.a[k];
            db[(size_t)p] = PT.b[k];
            const int64_t Va = (int64_t)PT.val[k] << e;
            c->apx.h_vapx[(size_t)c->wts.h_seq_perm[(size_t)p]] = Va;
            delta = std::max(delta, std::fabs((double)(Va - V)) / (double)V);
        }
    };
    assign(4);
    c->apx.apx_fine = false;
    if (delta > 1.5e-3) {
        assign(1);
        c->apx.apx_fine = true;
    }
    c->apx.apx_delta = delta;
    c->apx.apx_e_last = S4 > 0 ? em[(size_t)S4 - 1] : 0;
    c->apx.apx_transitions = transitions;
    // units of 2^e_last a GEMM entry can have lost to the truncations: < 1 unit of 2^e(m) at every transition into macro step m
    c->apx.apx_lost_units = 0;
    for (int k = 1; k < S4; ++k)
        if (sh[(size_t)k] > 0) c->apx.apx_lost_units += std::ldexp(1.0, em[(size_t)k] - c->apx.apx_e_last);
    const PopSegTables pop = build_pop_segs(Vp.data(), N, Npad);
    c->apx.n_pop_segs = pop.n_segs;
    c->apx.n_classes = pop.n_classes;
    if (int rc = c->apx.dig_a.reserve((size_t)Npad)) return rc;
    if (int rc = c->apx.dig_b.reserve((size_t)Npad)) return rc;
    if (int rc = c->apx.apx_shift.reserve((size_t)std::max(S4, 4) * 4)) return rc;
    if (int rc = c->apx.pop_segs.reserve(pop.segs.size() * sizeof(PopSeg))) return rc;
    if (int rc = c->apx.pop_wbeg.reserve(pop.wbeg.size() * 4)) return rc;
    if (int rc = c->apx.pop_vpos.reserve((size_t)Npad * 8)) return rc;
    LDW_HIP(hipMemcpyAsync(c->apx.pop_vpos.p, pop.vpos.data(), (size_t)Npad * 8, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(c->apx.dig_a.p, da.data(), (size_t)Npad, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(c->apx.dig_b.p, db.data(), (size_t)Npad, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(c->apx.apx_shift.p, sh.data(), (size_t)S4 * 4, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(c->apx.pop_segs.p, pop.segs.data(), pop.segs.size() * sizeof(PopSeg), hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(c->apx.pop_wbeg.p, pop.wbeg.data(), pop.wbeg.size() * 4, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));   // (the host vectors are on this frame)
    // The path pays when the approximation is tight enough for the screen to dismiss almost everything (its margin grows with
    // delta); the digit arrays of the GEMM must fit in LDS.  Any weights qualify: with many distinct values the popcount sums of
    // the listed pairs walk more segments per word, which is still cheap for the few pairs that are listed.
    // (r03 also required the popcount segment tables of k_pair_sums to fit 60 000 B of LDS, which switched the path off for ~3700 and more
    // distinct weights; the kernel now reads larger tables from global memory)
    c->apx.apx_ok = delta <= 4e-3 && Npad <= 30720 && M2 > 0;
    {
        char why[160];
        if (c->apx.apx_ok) snprintf(why, sizeof(why), c->apx.apx_fine ? "ok (block exponents per 32 positions)" : "ok");
        else if (!(delta <= 4e-3)) snprintf(why, sizeof(why), "delta %.3g > 4e-03 (dual-digit weights too coarse)", delta);
        else if (Npad > 30720) snprintf(why, sizeof(why), "Npad %lld > 30720 (digit arrays exceed the GEMM's LDS)", (long long)Npad);
        else snprintf(why, sizeof(why), "no macro step (Npad %lld)", (long long)Npad);
        c->apx.apx_gate = why;
    }
    return LDW_OK;
}

// ------------------------------------------------------------------------------------------------
// k_pack_panel: the 128 bits of macro step m of row-list position r as ONE 16-byte piece panel[m][r] (consecutive rows are
// consecutive pieces: the GEMM's loads are contiguous runs).  interleave != 0 (gemm_apx_kernel, one block exponent per k-step): the eight
// 16-bit groups g of the macro step are stored as word 0 = groups (0, 2, 4, 6), word 1 = groups (1, 3, 5, 7), so that the lane half fh of an
// MFMA k-step kk finds ITS sixteen positions 32 kk + 16 fh .. + 15 — a k-step covers 32 CONSECUTIVE positions, one block exponent —
// at bits 16 kk of word fh.  interleave == 0 (one exponent per macro step): the words as they are.
// Every word then goes out SCALED (r06) as FOUR dwords, dword kk = the word's bytes 2 kk and 2 kk + 1 each multiplied by 8 in a 16-bit field —
// the byte offsets of the two entries of the kernel's 8-byte expansion table that k-step kk looks up: the kernel gets an offset with ONE VALU
// instruction (and / shift) instead of two (extract, then scale); piece ((m Rpad + r) 2 + word) of 16 bytes, a panel twice the size.
// ------------------------------------------------------------------------------------------------
// blockIdx.y = 1: the second row list of the launch (rowlist2 / Rpad2 / panel2: the to side of an off-diagonal block — both panels in ONE launch).
__global__ __launch_bounds__(256) void k_pack_panel(const uint64_t *__restrict__ Mbits, int64_t KW, const int32_t *__restrict__ rowlist,
                                                    int Rpad, int M2, uint64_t *__restrict__ panel, int interleave,
                                                    const int32_t *__restrict__ rowlist2 = nullptr, int Rpad2 = 0, uint64_t *__restrict__ panel2 = nullptr) {
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    if (blockIdx.y == 1) {
        rowlist = rowlist2;
        Rpad = Rpad2;
        panel = panel2;
    }
    const int r = blockIdx.x * 64 + (threadIdx.x & 63);
    if (r >= Rpad) return;
    const u64x2 *src = reinterpret_cast<const u64x2 *>(Mbits + (int64_t)rowlist[r] * KW);
    u32x4 *dst4 = reinterpret_cast<u32x4 *>(panel);
    for (int m = threadIdx.x >> 6; m < M2; m += 4) {
        u64x2 v = src[m];
        if (interleave) {
            const unsigned long long x = v[0], y = v[1];
            // groups of x: g0 g1 g2 g3 (16 bits each, g0 lowest), of y: g4 g5 g6 g7
            const unsigned long long ex = (x & 0xFFFFull) | ((x >> 16) & 0xFFFF0000ull) | ((y & 0xFFFFull) << 32) | ((y << 16) & 0xFFFF000000000000ull);
            const unsigned long long ox = ((x >> 16) & 0xFFFFull) | ((x >> 32) & 0xFFFF0000ull) | (((y >> 16) & 0xFFFFull) << 32) | (y & 0xFFFF000000000000ull);
            v[0] = ex;   // g0 g2 g4 g6
            v[1] = ox;   // g1 g3 g5 g7
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned long long w = v[h];
            u32x4 o;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
                o[kk] = (((unsigned int)(w >> (16 * kk)) & 0xFFu) << 3) | (((unsigned int)(w >> (16 * kk + 8)) & 0xFFu) << 19);
            dst4[((int64_t)m * Rpad + r) * 2 + h] = o;
        }
    }
}

int launch_pack_panel(ldw_ctx *c, const int32_t *rowlist, int Rpad, uint64_t *panel, hipStream_t st, const int32_t *rowlist2, int Rpad2, uint64_t *panel2) {
    const int rmax = (rowlist2 && Rpad2 > Rpad) ? Rpad2 : Rpad;
    hipLaunchKernelGGL(k_pack_panel, dim3((unsigned)((rmax + 63) / 64), rowlist2 ? 2u : 1u), dim3(256), 0, st, c->rows.Mbits.as<uint64_t>(), c->KW, rowlist, Rpad,
                       (int)(c->KW / 2), panel, c->apx.apx_fine ? 1 : 0, rowlist2, Rpad2, panel2);
    LDW_HIP(hipGetLastError());
    return LDW_OK;
}

// ------------------------------------------------------------------------------------------------
// gemm_apx_kernel<MT, NT>: G'[t][f] = sum_p [row t has bit p][row f has bit p] a_p b_p 2^(e(p) - e_last), truncated at the
// exponent transitions (each loses < 1 unit).  256 threads = 4 independent waves (2 x 2), each with a tile of MT x NT MFMA
// tiles of 32 x 32 x 32 int8 (default 4 x 2 = 128 to-side x 64 from-side rows: 128 accumulator registers, everything in
// VGPRs so that the shift at an exponent transition is plain VALU, two waves per SIMD; with 4 x 4 tiles the accumulators
// have to live in AGPRs and hipcc 7.2 spills around the shift).  No LDS staging of the operand bits and no barrier in the
// K loop: every lane reads the 64-bit word of ITS row and lane half straight from the packed panel (consecutive rows are
// consecutive 16-B pieces: coalesced), one macro step ahead; LDS only holds the 0xFF expansion table and the two digit
// arrays.  Per MFMA k-step (32 positions) a lane expands 16 bits of each of its MT + NT rows through the table (2 look-ups
// each) and masks them with the 16 digits of its lane half: 6 (MT + NT) VALU + 2 (MT + NT) ds_read_b64 for MT NT MFMAs.
// r07: on the list launch a wave computes a RUN of tiles (ApxGemmArgs::grid_wgs): the workgroup stages LDS once, takes its one barrier, and every
// wave loops tile by tile on its own, the next tile's first panel pieces requested before the epilogue of the current one.
// ------------------------------------------------------------------------------------------------
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
// Wave tile of the pruned, table-fused launches (the default path's): APX_MT x 2 MFMA tiles of 32 x 32 = 128 to-rows x 64 from-rows, two waves per SIMD.
// (Measured and NOT kept, r02-r05 — numbers in docs/HISTORY.md and profiles/r05_*: 2 x 2 at four waves per SIMD, 3 x 2 at three, 3 x 3, 5 x 2; the table
// index as one SDWA instruction; the table reads one k-step ahead; a 16-way replicated table.  Their code left this file in r06: git history has it.)
constexpr int APX_MT = 4, APX_WPS = 2;

// the 16 expanded bytes (0xFF / 0x00) of the 16 bits of k-step KK: two look-ups in the 256-entry byte -> 8 x 0xFF table (LDS).  From a piece
// of the scaled panel (k_pack_panel): dword KK holds the two table offsets, in bytes, as 16-bit fields
typedef unsigned int apx_u32x4 __attribute__((ext_vector_type(4)));
template <int KK>
__device__ __forceinline__ v4i expand16s(const uint8_t *lut_bytes, const apx_u32x4 &w) {
    typedef unsigned long long u64x2v __attribute__((ext_vector_type(2)));
    const unsigned int d = w[KK];
    const u64x2v q = {*reinterpret_cast<const uint64_t *>(lut_bytes + (d & 0xFFFFu)), *reinterpret_cast<const uint64_t *>(lut_bytes + (d >> 16))};
    return __builtin_bit_cast(v4i, q);
}
constexpr int APX_LUT_BYTES = 2048;

// Epilogue of a wave tile (MT x NT MFMA tiles at wave-tile coordinates ty, tx): the threshold-table test per region of 32 to-rows x
// the wave's from-rows (P.fuse) and the store of the regions that are not clean.  s_bt: 256 wave-private LDS bytes.
template <int MT, int NT>
__device__ __forceinline__ void apx_gemm_epilogue(const ApxGemmArgs &P, v16i (&acc)[MT][NT], int ty, int tx, int lane, const int2 *s_tab, uint8_t *s_bt) {
    constexpr int TH = 32 * MT, TWd = 32 * NT;
    const int frow = lane & 31, fh = lane >> 5;
    int bf[NT];
    if (P.fuse) {
#pragma unroll
        for (int j = 0; j < NT; ++j) bf[j] = (int)P.bin_f[tx * TWd + 32 * j + frow];
        // one coalesced load of the wave tile's TH to-side bins, then LDS byte reads at static offsets (64 separate global byte
        // loads per lane made the epilogue cost more than the screen saved)
        for (int r = lane; r < TH; r += 64) s_bt[r] = P.bin_t[ty * TH + r];
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0);   // (wave-private LDS: the writes of this wave are done before its reads)
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        bool store = true;
        if (P.fuse) {   // region = to-rows [ty TH + 32 i, + 32) x the wave's from-rows (NT * 32 = 64 when NT = 2)
            bool ok = true;
#pragma unroll
            for (int j = 0; j < NT; ++j) ok = ok && bf[j] != 255;
            if (P.sr_mask && P.sr_mask[(int64_t)((ty * TH) / 128) * (P.RFpad / 64) + tx] != 0) ok = false;   // (the band mask's tiles are 128 x 64; TWd = 64)
            int bt[16];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                bt[e] = (int)s_bt[32 * i + (e & 3) + 8 * (e >> 2) + 4 * fh];
                ok = ok && bt[e] != 255;
            }
            unsigned int fails = 0;   // bit e * NT + j: entry outside its thresholds
            const bool eligible = __ballot(!ok) == 0ull;
            if (eligible) {   // (a region with a row of another kind of SNP is stored without the 32 look-ups per lane)
#pragma unroll
                for (int e = 0; e < 16; ++e)
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        const int2 th = s_tab[bt[e] * P.tab_nb + bf[j]];
                        const int n = acc[i][j][e];
                        const bool in = n > th.x && n < th.y;
                        ok = ok && in;
                        if (!in) fails |= 1u << (e * NT + j);
                    }
            }
            if (NT == 2 && P.maybe && eligible && __ballot(!ok) != 0ull) {
                // r04: the few entries outside their thresholds go to the maybe list, the region counts as clean
                const unsigned int mine = (unsigned int)__popc(fails);
                unsigned int incl = mine;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const unsigned int t = __shfl_up(incl, o);
                    if (lane >= o) incl += t;
                }
                const unsigned int tot = (unsigned int)__builtin_amdgcn_readlane((int)incl, 63);
                if (tot <= (unsigned int)APX_MAYBE_MAX) {
                    unsigned int base = 0;
                    if (lane == 0) base = atomicAdd(P.maybe_n, tot);
                    base = (unsigned int)__builtin_amdgcn_readfirstlane((int)base);
                    unsigned int pos = base + incl - mine;
                    unsigned int f = fails;
                    while (f) {
                        const int b = __builtin_ctz(f);
                        f &= f - 1;
                        const int e = b / NT, j = b % NT;
                        if (pos < P.maybe_cap) {
                            ApxMaybe m;
                            m.trow = (uint32_t)(ty * TH + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * fh);
                            m.fcol = (uint32_t)(tx * TWd + 32 * j + frow);
                            // (dynamic index into the accumulator tile: a select chain over the 32 candidates, only on this rare path)
                            int v = 0;
#pragma unroll
                            for (int ee = 0; ee < 16; ++ee)
#pragma unroll
                                for (int jj = 0; jj < NT; ++jj) v = (ee == e && jj == j) ? acc[i][jj][ee] : v;
                            m.n = v;
                            P.maybe[pos] = m;
                        }
                        ++pos;
                    }
                    ok = true;   // handled: clean
                }
            }
#ifdef LDW_ABLATE_GEMM_STORE   // timing ablation only (wrong results): what the G' stores of the table-eligible regions that are not clean cost
            const bool clean = __ballot(bf[0] == 255 || bt[0] == 255) == 0ull || __ballot(!ok) == 0ull;
#else
            const bool clean = __ballot(!ok) == 0ull;
#endif
            if (lane == 0) {
#pragma unroll
                for (int h = 0; h < (NT * 32) / 64; ++h) P.clean[(int64_t)((ty * TH + 32 * i) / 32) * (P.RFpad / 64) + (tx * TWd) / 64 + h] = clean ? 1 : 0;
            }
            store = !clean;
        }
        if (store) {
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int fcol = tx * TWd + 32 * j + frow;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int trow = ty * TH + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * fh;
                    P.G[(int64_t)trow * P.RFpad + fcol] = acc[i][j][e];
                }
            }
        }
    }
}

// Tile pruning (ApxGemmArgs::skip_ctr).  k_apx_live_tiles: which wave tiles (128 to-rows x 64 from-rows) does the approximate GEMM have
// to compute?  A tile is pruned when EVERY pair in it is dismissed whatever its joint count:
//   (a) all rows carry bins of the threshold table and the rectangle [min, max] x [min, max] of their bins holds only unconditional
//       entries (-1, INT_MAX) — the epilogue's test n' > L && n' < H would pass whatever the GEMM computed.  The rows of a block are
//       ordered by their marginal (prep_block), so a tile spans a few bins per side (rectangles of more than 64 entries: computed);
//   (b) the rows of each side are all of ONE kind (2 or 3 flagged states) and one side is dead versus the other's kind (k_snp_sup).
// One workgroup per 128-row group of the to side, one THREAD per tile: it folds the bins / flags of its 64 from-rows and of the
// group's 128 to-rows (16-byte loads).  Pruned tiles are flagged clean where that applies and counted; the others are appended to
// the list the GEMM runs over — in order within the group, ONE atomic per workgroup for the place of its run (a wave per tile with
// an atomic each took 130 us for the 16.6k tiles of a C4 block; this takes a few).
struct TileSummary {
    int bmin, bmax;
    unsigned fand, forr;
};
__device__ __forceinline__ TileSummary apx_fold_rows(const uint8_t *__restrict__ bins, const uint8_t *__restrict__ flags, int n) {
    TileSummary S{255, 0, 0xFFu, 0u};
    for (int i = 0; i < n; i += 16) {
        const uint4 b = *reinterpret_cast<const uint4 *>(bins + i);
        const unsigned w[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int v = (int)((w[k >> 2] >> (8 * (k & 3))) & 0xFFu);
            S.bmin = v < S.bmin ? v : S.bmin;
            S.bmax = v > S.bmax ? v : S.bmax;
        }
        if (flags) {
            const uint4 f = *reinterpret_cast<const uint4 *>(flags + i);
            unsigned a = f.x & f.y & f.z & f.w, o = f.x | f.y | f.z | f.w;
            a &= a >> 16; a &= a >> 8;
            o |= o >> 16; o |= o >> 8;
            S.fand &= a & 0xFFu;
            S.forr |= o & 0xFFu;
        }
    }
    return S;
}

__global__ __launch_bounds__(256) void k_apx_live_tiles(ApxGemmArgs P) {
    constexpr int MT = APX_MT, NT = 2, TH = 32 * MT, TWd = 32 * NT;
    __shared__ unsigned int s_wave[4], s_base;
    const int ty = (int)blockIdx.x, ntx = P.RFpad / TWd;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const TileSummary T = apx_fold_rows(P.bin_t + (int64_t)ty * TH, P.rflag_t ? P.rflag_t + (int64_t)ty * TH : nullptr, TH);
    unsigned int n_pruned = 0;
    for (int tx0 = 0; tx0 < ntx; tx0 += 256) {
        const int tx = tx0 + (int)threadIdx.x;
        // (a diagonal block: the tiles above the diagonal of row positions are not part of the GEMM at all — their regions keep the zero the host set)
        const bool valid = tx < ntx && !(P.lower_only && tx * TWd + TWd - 1 < ty * TH);
        bool pruned = false, all_binned = false;
        if (valid && !(P.sr_mask && P.sr_mask[(int64_t)((ty * TH) / 128) * (P.RFpad / 64) + tx] != 0)) {
            const TileSummary F = apx_fold_rows(P.bin_f + (int64_t)tx * TWd, P.rflag_f ? P.rflag_f + (int64_t)tx * TWd : nullptr, TWd);
            all_binned = T.bmax < P.tab_nb && F.bmax < P.tab_nb;
            if (P.rflag_t) {   // the wider tables: rows of ONE kind per side, one side dead versus the other's kind (k_snp_sup)
                const unsigned kt = T.fand & PF_KIND, kf = F.fand & PF_KIND;
                pruned = kt >= 2u && kt == (T.forr & PF_KIND) && kf >= 2u && kf == (F.forr & PF_KIND) &&
                         ((T.fand & (kf == 2u ? PF_DEAD2 : PF_DEAD3)) != 0u || (F.fand & (kt == 2u ? PF_DEAD2 : PF_DEAD3)) != 0u);
            }
            if (!pruned && all_binned && (T.bmax - T.bmin + 1) * (F.bmax - F.bmin + 1) <= 64) {   // the table: only unconditional entries
                bool ok = true;
                for (int bt = T.bmin; bt <= T.bmax; ++bt)
                    for (int bf = F.bmin; bf <= F.bmax; ++bf) {
                        const int2 th = P.tab[bt * P.tab_nb + bf];
                        ok = ok && th.x < 0 && th.y == 2147483647;
                    }
                pruned = ok;
            }
        }
        if (pruned && all_binned) {
            // (clean flags speak of biallelic x biallelic regions only: k_mi_screen maps a region to a tile and 32 column slots by row
            // position, which holds there; the other pruned tiles are found again by the screen from the SNPs' flags)
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int h = 0; h < (NT * 32) / 64; ++h) P.clean[(int64_t)((ty * TH + 32 * i) / 32) * (P.RFpad / 64) + (tx * TWd) / 64 + h] = 1;
        }
        const bool live = valid && !pruned;
        const unsigned long long lm = __ballot(live);
        n_pruned += (unsigned int)__popcll(__ballot(valid && pruned));
        if (lane == 0) s_wave[wave] = (unsigned int)__popcll(lm);
        __syncthreads();
        if (threadIdx.x == 0) {
            const unsigned int tot = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
            s_base = tot ? atomicAdd(P.n_live, tot) : 0u;
        }
        __syncthreads();
        unsigned int off = s_base;
        for (int w = 0; w < wave; ++w) off += s_wave[w];
        if (live) P.tile_list[off + (unsigned int)__popcll(lm & ((1ull << lane) - 1ull))] = (uint32_t)(ty * ntx + tx);
        __syncthreads();
    }
    if (lane == 0 && n_pruned) atomicAdd(P.skip_ctr, (unsigned long long)n_pruned);
}

template <int MT, int NT, bool FINE, int WPS = 2>
__global__ __launch_bounds__(256, WPS) void gemm_apx_kernel(ApxGemmArgs P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint64_t *lutFF = reinterpret_cast<uint64_t *>(smem);           // [256]: byte of bits -> 8 bytes of 0xFF / 0x00
    uint8_t *sA = smem + APX_LUT_BYTES, *sB = sA + (size_t)P.M2 * 128;       // digits by position
    int2 *s_tab = reinterpret_cast<int2 *>(sB + (size_t)P.M2 * 128);  // threshold table (P.fuse)
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int TH = 32 * MT, TWd = 32 * NT;
    const int ntx = P.RFpad / TWd;
    // The wave's run of tiles: entries k, k + step, ... < k_end of the live-tile list, or (2-D launch) the one tile of its place in the grid.
    // t: the tile's number ty * ntx + tx, -1: the wave has none.  All wave-uniform: they live in scalar registers.
    unsigned int k = 0, k_end = 0, step = 1;
    int t;
    if (P.tile_list) {
        // tile pruning (k_apx_live_tiles): the grid is 1-D over the list of the tiles that are left, four waves per workgroup; the workgroups
        // beyond the list (the worst-case grid, a short list) leave at once, before anything is staged
        const unsigned int n_live = *P.n_live, nw = gridDim.x * 4u, w = blockIdx.x * 4u + (unsigned int)wave;
        if (blockIdx.x * 4u >= n_live) return;
#ifdef LDW_APX_RUNS_CONTIG   // measurement only (same results): a run of consecutive entries per wave instead of every nw-th
        const unsigned int base = n_live / nw, rem = n_live % nw;
        k = w * base + (w < rem ? w : rem);
        k_end = k + base + (w < rem ? 1u : 0u);
#else
        // every nw-th entry: the waves in flight cover ONE window of the list that moves along it, as the dispatch order of the one-tile launch
        // does — neighbouring waves share their to-rows, the window's panel rows stay in L2
        k = w;
        k_end = n_live;
        step = nw;
#endif
        t = k < k_end ? (int)P.tile_list[k] : -1;
    } else {
        auto outside = [&](int ty, int tx) { return ty * TH >= P.RTpad || tx * TWd >= P.RFpad || (P.lower_only && tx * TWd + TWd - 1 < ty * TH); };
        const int ty0 = 2 * (int)blockIdx.y, tx0 = 2 * (int)blockIdx.x;
        // (a diagonal block: the workgroups wholly above the diagonal — about half the grid — leave before they stage anything)
        if (outside(ty0, tx0) && outside(ty0, tx0 + 1) && outside(ty0 + 1, tx0) && outside(ty0 + 1, tx0 + 1)) return;
        const int ty = ty0 + (wave >> 1), tx = tx0 + (wave & 1);
        t = outside(ty, tx) ? -1 : ty * ntx + tx;
    }
    // staged ONCE per workgroup, whatever the length of its waves' runs
    if (P.fuse)
        for (int i = tid; i < P.tab_nb * P.tab_nb; i += 256) s_tab[i] = P.tab[i];
    {
        uint64_t e = 0;
#pragma unroll
        for (int k8 = 0; k8 < 8; ++k8) e |= ((tid >> k8) & 1) ? (0xFFull << (8 * k8)) : 0ull;
        lutFF[tid] = e;
        const int n16 = P.M2 * 8;   // 16-byte pieces per digit array
        for (int i = tid; i < n16; i += 256) {
            reinterpret_cast<uint4 *>(sA)[i] = reinterpret_cast<const uint4 *>(P.dig_a)[i];
            reinterpret_cast<uint4 *>(sB)[i] = reinterpret_cast<const uint4 *>(P.dig_b)[i];
        }
    }
    __syncthreads();   // the only barrier: none inside the tile loop
    if (t < 0) return;
    const int frow = lane & 31, fh = lane >> 5;
    const int64_t sta = (int64_t)P.RTpad * 2, stb = (int64_t)P.RFpad * 2;
    // Pieces of the scaled panel (k_pack_panel).  ONE pointer per side — the lane's piece of the tile's first row at macro step 0; the MFMA tile 32 i is
    // an immediate offset (32 rows of 2 pieces of 16 bytes) — so that the next tile's addressing costs the epilogue four registers, not twelve.
    // (A wave-uniform base with a 32-bit lane offset would cost none: hipcc 7.2's register allocator crashes on it under the iterative-ilp scheduler.)
    const uint8_t *base_t, *base_f;
    const unsigned int lane_off = (unsigned int)(frow * 2 + fh) * 16u;
    auto piece = [&](const uint8_t *base, int64_t macro_step_bytes, int i) {
        return *reinterpret_cast<const apx_u32x4 *>(base + macro_step_bytes + 1024 * i);
    };
    apx_u32x4 wa[MT], wb[NT], na[MT], nb[NT];
    // tile (ty, tx): its place in the panels and the request for its first pieces
    auto open_tile = [&](int ty, int tx) {
        base_t = reinterpret_cast<const uint8_t *>(P.panel_t) + (int64_t)ty * TH * 32 + lane_off;
        base_f = reinterpret_cast<const uint8_t *>(P.panel_f) + (int64_t)tx * TWd * 32 + lane_off;
#pragma unroll
        for (int i = 0; i < MT; ++i) na[i] = piece(base_t, 0, i);
#pragma unroll
        for (int i = 0; i < NT; ++i) nb[i] = piece(base_f, 0, i);
    };
    const uint8_t *lut_bytes = smem;
    int ty = t / ntx, tx = t - ty * ntx;
    open_tile(ty, tx);
    for (;;) {
        // the next tile of the run, asked for now and looked at after the K loop
        k += step;
        const int t_next = k < k_end ? (int)P.tile_list[k] : -1;
        v16i acc[MT][NT];
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0;
        for (int m = 0; m < P.M2; ++m) {
#pragma unroll
            for (int i = 0; i < MT; ++i) wa[i] = na[i];
#pragma unroll
            for (int i = 0; i < NT; ++i) wb[i] = nb[i];
            if (m + 1 < P.M2) {
#pragma unroll
                for (int i = 0; i < MT; ++i) na[i] = piece(base_t, (int64_t)(m + 1) * sta * 16, i);
#pragma unroll
                for (int i = 0; i < NT; ++i) nb[i] = piece(base_f, (int64_t)(m + 1) * stb * 16, i);
            }
            // FINE: one block exponent per k-step; k-step kk = positions 128 m + 32 kk .. + 31 (k_pack_panel interleaves the panel words
            // accordingly), lane half fh holds 16 of them.  Coarse (the weights' dynamic range within 128 positions is small: clonal
            // data): one exponent per macro step, k-step kk = bits 16 kk of the plain words 0 and 1 — 4 % faster (0.517 vs 0.538 ms).
            // (wave-uniform: one scalar load per macro step.  Read through the constant address space — nothing writes the shifts while the kernel runs —
            // because the stores of the previous tile's epilogue now precede the load, and a load they might alias becomes a VECTOR load with a wait
            // for everything in flight, the next step's panel pieces included: +6 % on the kernel)
            typedef const __attribute__((address_space(4))) v4i *shift_ptr;
            const v4i sh4 = ((shift_ptr)(uintptr_t)P.shift)[m];
            const int shk[4] = {sh4[0], sh4[1], sh4[2], sh4[3]};
            const uint8_t *dA = sA + m * 128 + fh * (FINE ? 16 : 64), *dB = sB + m * 128 + fh * (FINE ? 16 : 64);
            auto kstep = [&](auto KKc) {
                constexpr int kk = decltype(KKc)::value;
                const int sh = shk[kk];
                if ((FINE || kk == 0) && sh) {
#pragma unroll
                    for (int i = 0; i < MT; ++i)
#pragma unroll
                        for (int j = 0; j < NT; ++j)
#pragma unroll
                            for (int e = 0; e < 16; ++e) acc[i][j][e] = (int)((unsigned)acc[i][j][e] >> sh);
                }
                const v4i da = *reinterpret_cast<const v4i *>(dA + (FINE ? 32 : 16) * kk);
                const v4i db = *reinterpret_cast<const v4i *>(dB + (FINE ? 32 : 16) * kk);
                v4i fa[MT], fb[NT];
#pragma unroll
                for (int i = 0; i < MT; ++i) fa[i] = expand16s<kk>(lut_bytes, wa[i]) & da;
#pragma unroll
                for (int i = 0; i < NT; ++i) fb[i] = expand16s<kk>(lut_bytes, wb[i]) & db;
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
            };
            kstep(std::integral_constant<int, 0>{});
            kstep(std::integral_constant<int, 1>{});
            kstep(std::integral_constant<int, 2>{});
            kstep(std::integral_constant<int, 3>{});
        }
        // the first pieces of the next tile are on their way while the epilogue tests and stores this one (na / nb are free after the last macro step)
        const int ty_next = t_next / ntx, tx_next = t_next - ty_next * ntx;
        if (t_next >= 0) open_tile(ty_next, tx_next);
        // (the empty statement makes the offset a value of THIS pass of the loop: the epilogue's sixteen LDS addresses are then made here, per tile, as
        // before; hoisted out of the tile loop they lived through the K loop and two registers spilled)
        int bt_off = wave * 256;
        asm volatile("" : "+s"(bt_off));
        apx_gemm_epilogue<MT, NT>(P, acc, ty, tx, lane, s_tab, reinterpret_cast<uint8_t *>(s_tab + 64 * 64) + bt_off);
        if (t_next < 0) break;
        ty = ty_next;
        tx = tx_next;
    }
}

int launch_apx_live_tiles(ldw_ctx *c, const ApxGemmArgs &P, hipStream_t st) {
    LDW_REQUIRE(P.fuse && P.skip_ctr && P.tile_list && P.n_live && P.RTpad % 128 == 0 && P.RFpad % 64 == 0 && P.tab && P.tab_nb == 64,
                LDW_ERR_ARG, "launch_apx_live_tiles: bad pruning arguments");
    hipLaunchKernelGGL(k_apx_live_tiles, dim3((unsigned)(P.RTpad / (32 * APX_MT))), dim3(256), 0, st, P);
    LDW_HIP(hipGetLastError());
    return LDW_OK;
}

int launch_gemm_apx(ldw_ctx *c, const ApxGemmArgs &P, hipStream_t st) {
    LDW_REQUIRE(P.RTpad % APX_TW == 0 && P.RFpad % APX_TW == 0 && P.M2 > 0, LDW_ERR_ARG, "launch_gemm_apx: padding violated (RT %d RF %d M2 %d)", P.RTpad,
                P.RFpad, P.M2);
    const size_t lds = APX_LUT_BYTES + (size_t)P.M2 * 256 + (P.fuse ? (size_t)P.tab_nb * P.tab_nb * 8 + 1024 : 0);
    LDW_REQUIRE(lds <= 65536, LDW_ERR_ARG, "launch_gemm_apx: %d positions do not fit the LDS digit arrays", P.M2 * 128);
    LDW_REQUIRE(!P.fuse || (P.tab_nb == 64 && P.bin_t && P.bin_f && P.tab && P.clean), LDW_ERR_ARG, "launch_gemm_apx: bad table arguments");
    LDW_REQUIRE(!P.skip_ctr || (P.fuse && P.tile_list), LDW_ERR_ARG, "launch_gemm_apx: bad pruning arguments");
    if (P.tile_list) {   // (the list is made by launch_apx_live_tiles, or by the caller: ldw_debug_apx_gemm_list)
        LDW_REQUIRE(P.n_live && P.RFpad % 64 == 0 && P.grid_wgs >= 0, LDW_ERR_ARG, "launch_gemm_apx: bad tile list arguments");
        const int tiles = (P.RTpad / (32 * APX_MT)) * (P.RFpad / 64), worst = (tiles + 3) / 4;
        const int g = P.grid_wgs > 0 ? P.grid_wgs : worst;
        if (P.fine) hipLaunchKernelGGL((gemm_apx_kernel<APX_MT, 2, true, APX_WPS>), dim3((unsigned)g), dim3(256), lds, st, P);
        else hipLaunchKernelGGL((gemm_apx_kernel<APX_MT, 2, false, APX_WPS>), dim3((unsigned)g), dim3(256), lds, st, P);
    } else {
        const int ntx = P.RFpad / 64, nty = P.RTpad / 128;
        const dim3 grid((unsigned)((ntx + 1) / 2), (unsigned)((nty + 1) / 2));
        if (P.fine) hipLaunchKernelGGL((gemm_apx_kernel<4, 2, true>), grid, dim3(256), lds, st, P);
        else hipLaunchKernelGGL((gemm_apx_kernel<4, 2, false>), grid, dim3(256), lds, st, P);
    }
    LDW_HIP(hipGetLastError());
    {   // executed work (ldw_gemm_stats): waves that do not leave at once, each 2 * rows_t * rows_f * K int8 operations
        constexpr int TH = 128, TWd = 64;
        int64_t waves = 0;
        for (int ty = 0; ty * TH < P.RTpad; ++ty) {
            const int ntx = P.RFpad / TWd;
            if (!P.lower_only) waves += ntx;
            else for (int tx = 0; tx < ntx; ++tx) waves += (tx * TWd + TWd - 1 < ty * TH) ? 0 : 1;
        }
        c->cnt.gemm_stat[0] += 1;
        if (P.fuse) c->cnt.gemm_stat[5] += 1;
        c->cnt.gemm_stat[1] += 2.0 * (double)waves * TH * TWd * ((double)P.M2 * 128.0);
        if (P.fuse && P.skip_ctr) {   // the tiles the kernel prunes are taken off again when the counter is read (ldw_gemm_stats, ldw_links_end)
            c->apx_ops_per_wave = 2.0 * TH * TWd * ((double)P.M2 * 128.0);
            c->cnt.apx_waves_total += waves;
        }
    }
    return LDW_OK;
}

// Workgroups per resident slot of the list launch (two slots per CU: APX_WPS waves per SIMD).  1 would be fully persistent: fewest turnovers, but the
// main stream's short kernels get onto a CU only where a GEMM workgroup retires.  Chosen by the overlapped pass's time: profiles/r07_apx_tile_runs.txt.
constexpr int APX_RUNS_R = 8;

int apx_run_grid(const ldw_ctx *c, int RTpad, int RFpad) {
    if (getenv("LDW_NO_APX_RUNS") != nullptr) return 0;   // (read per call: the tests switch it)
    if (const char *e = getenv("LDW_APX_GRID_WGS")) {
        const int k = atoi(e);
        if (k > 0) return k;
    }
    const int worst = ((RTpad / (32 * APX_MT)) * (RFpad / 64) + 3) / 4;
    return std::max(1, std::min(worst, APX_RUNS_R * APX_WPS * std::max(c->n_cu, 1)));
}

void warm_apx() {   // ldw_ctx_reserve: load this translation unit's code object ahead of its first launch
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_pack_panel));
    (void)hipGetLastError();
}
}  // namespace ldw
