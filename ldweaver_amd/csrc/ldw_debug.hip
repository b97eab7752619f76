// Test hooks (r06): the engine's BOUNDS as functions.  The default path dismisses pairs on hand-derived bounds (BOUNDS.md); each of them is
// reachable here WITHOUT running a pass, on caller-made inputs, so that tests/test_bounds.py can brute-force it against the MI formula of
// src/computeMI.cpp:19 — random and extremal joint tables, quirk Q1's RXY != r_a r_b / 4, the engine's own constants:
//   ldw_debug_apx_params    the dual-digit weights V' of the current weighting and every constant the approximate screen's bound is built from
//   ldw_debug_rows          SNP -> indicator rows (which state each row stands for)
//   ldw_debug_apx_gemm      gemm_apx_kernel on caller-chosen rows: the int32 sums G' (truncation bound apx_lost_units)
//   ldw_debug_apx_gemm_fused  the FUSED launches of the default path (launch_pack_panel, launch_apx_live_tiles, launch_gemm_apx with P.fuse = 1) on caller-made rows, bins,
//                           row flags, threshold table and band mask: the raw G', clean flags, live-tile list, maybe list and counters, each over a fill pattern
//   ldw_debug_limb_gemm     launch_gemm_bits / launch_cooc_popc on caller-chosen rows, limbs, strips, masks and tile lists: the exact int64 sums, every entry the launch left alone
//   ldw_debug_lo_units      launch_gemm_lo_units on caller-made unit lists, laid out by lo_layout (ldw_lo_geom.h) as prep_block lays out a block: the raw low-limb buffer
//   ldw_debug_pair_sums     the exact sums of caller-made pair lists through launch_pair_sums (every form, a forced grid), without k_pair_mi
//   ldw_debug_screen_bound  full_cells_screen / pair_screen_generic (fp32; APX and exact-limb forms) and full_cells_mi (fp64) on caller-made tables
// Nothing here is on the product path; the kernels are the product's own device functions (ldw_epi.h), instantiated once more.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ldw_apx.h"
#include "ldw_pairs.h"
#include "ldw_dev.h"
#include "ldw_gemm_tile.h"

using namespace ldw;

namespace ldw {

struct DbgArrays {
    const int64_t *g;      // [n][4][4]: joint sums of the indicator rows, g[case][j][i] (slot i of the from-side SNP, slot j of the to-side SNP)
    const int32_t *g32;    // the same as int32 (approximate path)
    const int64_t *pa, *pb;   // [n][5] integer marginals by slot (units of the sums)
    const float *pX, *pY;     // [n][5] weighted marginals by slot (weight units)
    const double *rr;         // [n][3]: r_a, r_b, RXY
    const uint32_t *mk;       // [n][2]: slot meta of the two SNPs (rows | uqe flags << 3), generic kinds only
    float *out;
    double *out64;
    int64_t n;
};

template <int NA, int NB>
__device__ __forceinline__ void dbg_sides(const DbgArrays &D, int64_t k, RowSide &R, ColMeta &M) {
    R.ra = D.rr[k * 3 + 0];
    M.rb = D.rr[k * 3 + 1];
    R.rta = M.rq = 0.0;
    R.ra0 = 0;
    M.rb0 = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        R.pa[i] = D.pa[k * 5 + i];
        M.pb[i] = D.pb[k * 5 + i];
        R.pXf[i] = D.pX[k * 5 + i];
        M.pYf[i] = D.pY[k * 5 + i];
        R.pXd[i] = (double)R.pXf[i];
        M.pYd[i] = (double)M.pYf[i];
    }
    R.na = NA;
    R.ma = (uint32_t)NA | (((2u << NA) - 1u) << 3);
    M.mb = (uint32_t)NB | (((2u << NB) - 1u) << 3);
}

// kind 0: the approximate path's multi-cell bound, exactly as screen_cols_apx evaluates it (full_cells32 -> full_cells_screen<.., true>);
// kind 2: the exact-limb screen (full_cells -> full_cells_screen<.., false>: the value is an fp32 MI, no bound terms)
template <int NA, int NB, int KIND>
__global__ __launch_bounds__(256) void k_dbg_full(EpiArgs A, DbgArrays D) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= D.n) return;
    RowSide R;
    ColMeta M;
    dbg_sides<NA, NB>(D, k, R, M);
    const double rxy = D.rr[k * 3 + 2];
    if (KIND == 0) {
        int raw[NB][NA];
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int i = 0; i < NA; ++i) raw[j][i] = D.g32[k * 16 + j * 4 + i];
        FullCells32<NA, NB> C;
        full_cells32<NA, NB>(R, M, raw, C);
        D.out[k] = full_cells_screen<NA, NB, true>(A, R, M, rxy, C);
    } else {
        const GAcc Ga = gacc_plain(D.g + k * 16, 1, 4);
        FullCells<NA, NB> C;
        full_cells<NA, NB>(R, M, Ga, C);
        if (KIND == 2) D.out[k] = full_cells_screen<NA, NB, false>(A, R, M, rxy, C);
        else {   // KIND 4: the fp64 evaluation of the emitted value (full_cells_mi) — marginals in double from the integer ones, as load_row_side makes them
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                R.pXd[i] = (double)R.pa[i] * A.scale;
                M.pYd[i] = (double)M.pb[i] * A.scale;
            }
            D.out64[k] = full_cells_mi<NA, NB>(A, R, M, rxy, C);
        }
    }
}

// kinds 1 / 3: the predicated screens of SNPs with any slot counts and unflagged slots (pair_screen_generic<APX>)
template <bool APX>
__global__ __launch_bounds__(256) void k_dbg_generic(EpiArgs A, DbgArrays D) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= D.n) return;
    RowSide R;
    ColMeta M;
    dbg_sides<1, 1>(D, k, R, M);
    R.ma = D.mk[k * 2 + 0];
    M.mb = D.mk[k * 2 + 1];
    R.na = (int)(R.ma & 7);
    GAcc Ga = gacc_plain(APX ? reinterpret_cast<const int64_t *>(D.g32 + k * 16) : D.g + k * 16, 1, 4);
    Ga.w32 = APX ? 1 : 0;
    D.out[k] = pair_screen_generic<APX>(A, R, M, D.rr[k * 3 + 2], Ga);
}

}  // namespace ldw

extern "C" {

int ldw_debug_apx_params(ldw_ctx *c, double out[20], int64_t *vfixed_out, int64_t *vapx_out, int64_t capacity) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(out, LDW_ERR_ARG, "ldw_debug_apx_params: null output");
    LDW_REQUIRE(c->wts.have_weights, LDW_ERR_STATE, "ldw_debug_apx_params: no weights (ldw_set_weights)");
    EmitArgs E;
    memset(&E, 0, sizeof(E));
    apx_screen_params(c, E);
    out[0] = c->wts.frac_bits;
    out[1] = c->apx.apx_e_last;
    out[2] = c->apx.apx_delta;
    out[3] = c->apx.apx_lost_units;
    out[4] = (double)c->wts.total_fixed;
    out[5] = c->wts.neff;
    out[6] = E.apx_EG;
    out[7] = E.apx_dfac;
    out[8] = E.apx_s1;
    out[9] = E.apx_c1;
    out[10] = E.apx_W;
    out[11] = E.apx_unit;
    out[12] = E.scr_scale;
    {   // the exact-limb screen reads the top 31 bits of a sum (make_emit_args, all limbs in the block-wide GEMM)
        int bits = 0;
        while (bits < 62 && (c->wts.total_fixed >> bits) != 0) ++bits;
        const int shift = bits > 31 ? bits - 31 : 0;
        out[13] = shift;
        out[14] = std::ldexp(1.0, shift - c->wts.frac_bits);
    }
    out[15] = (c->apx.apx_ok ? 1 : 0) | (c->apx.apx_fine ? 2 : 0);
    out[16] = c->wts.lo_abs_sum;   // mixed-precision path: sum_s |V_lo,s| 2^-F and the margin it adds to the screen (lo_bound, ldw_mi_items.inc)
    {
        const double den = c->wts.neff > 1.0 ? c->wts.neff : 1.0;
        out[17] = c->wts.lo_abs_sum * (2.0 * std::log(den + 12.5) + 3.0) / den;
    }
    out[18] = E.apx_MU;
    out[19] = c->wts.nlimbs;
    if (vfixed_out || vapx_out) {
        LDW_REQUIRE(capacity >= c->N, LDW_ERR_SIZE, "ldw_debug_apx_params: capacity %lld < N %lld", (long long)capacity, (long long)c->N);
        for (int64_t s = 0; s < c->N; ++s) {
            if (vfixed_out) vfixed_out[s] = c->wts.h_vfixed[(size_t)s];
            if (vapx_out) vapx_out[s] = (size_t)s < c->apx.h_vapx.size() ? c->apx.h_vapx[(size_t)s] : 0;
        }
    }
    return LDW_OK;
}

int ldw_debug_rows(ldw_ctx *c, int32_t *row0_out, uint32_t *slot_meta_out, int64_t capacity) {
    if (int rc = check_gpu(c)) return rc;
    if (int rc = ensure_rows(c)) return rc;
    LDW_REQUIRE(row0_out && slot_meta_out && capacity >= c->L + 1, LDW_ERR_ARG, "ldw_debug_rows: need L + 1 = %lld entries", (long long)c->L + 1);
    memcpy(row0_out, c->rows.h_row0.data(), (size_t)(c->L + 1) * 4);
    memcpy(slot_meta_out, c->rows.h_slot_meta.data(), (size_t)c->L * 4);
    return LDW_OK;
}

// grid_wgs < 0: the 2-D launch (ldw_debug_apx_gemm); > 0: the list launch over a list of every tile that holds an entry of `out`, with that grid
static int debug_apx_gemm(ldw_ctx *c, const int32_t *rows_t, int nrt, const int32_t *rows_f, int nrf, int grid_wgs, int32_t *out);

int ldw_debug_apx_gemm(ldw_ctx *c, const int32_t *rows_t, int nrt, const int32_t *rows_f, int nrf, int32_t *out) {
    return debug_apx_gemm(c, rows_t, nrt, rows_f, nrf, -1, out);
}

int ldw_debug_apx_gemm_list(ldw_ctx *c, const int32_t *rows_t, int nrt, const int32_t *rows_f, int nrf, int grid_wgs, int32_t *out) {
    LDW_REQUIRE(grid_wgs > 0 && grid_wgs <= 65536, LDW_ERR_ARG, "ldw_debug_apx_gemm_list: grid of %d workgroups outside 1..65536", grid_wgs);
    return debug_apx_gemm(c, rows_t, nrt, rows_f, nrf, grid_wgs, out);
}

static int debug_apx_gemm(ldw_ctx *c, const int32_t *rows_t, int nrt, const int32_t *rows_f, int nrf, int grid_wgs, int32_t *out) {
    if (int rc = check_gpu(c)) return rc;
    if (int rc = join_prepare(c)) return rc;
    if (int rc = ensure_rows(c)) return rc;
    LDW_REQUIRE(rows_t && rows_f && out && nrt > 0 && nrf > 0 && nrt <= 8192 && nrf <= 8192, LDW_ERR_ARG, "ldw_debug_apx_gemm: bad argument");
    LDW_REQUIRE(c->apx.apx_ok, LDW_ERR_STATE, "ldw_debug_apx_gemm: the weights do not allow the approximate path (%s)", c->apx.apx_gate.c_str());
    for (int k = 0; k < nrt; ++k) LDW_REQUIRE(rows_t[k] >= 0 && rows_t[k] <= c->rows.R, LDW_ERR_ARG, "ldw_debug_apx_gemm: to-side row %d = %d outside 0..R", k, rows_t[k]);
    for (int k = 0; k < nrf; ++k) LDW_REQUIRE(rows_f[k] >= 0 && rows_f[k] <= c->rows.R, LDW_ERR_ARG, "ldw_debug_apx_gemm: from-side row %d = %d outside 0..R", k, rows_f[k]);
    const int RTpad = (nrt + APX_TW - 1) / APX_TW * APX_TW, RFpad = (nrf + APX_TW - 1) / APX_TW * APX_TW, M2 = (int)(c->KW / 2);
    std::vector<int32_t> rl((size_t)RTpad + RFpad, (int32_t)c->rows.R);   // padding -> the all-zero row R
    std::copy(rows_t, rows_t + nrt, rl.begin());
    std::copy(rows_f, rows_f + nrf, rl.begin() + RTpad);
    DevBuf d_rl, d_pt, d_pf, d_G, d_list;
    std::vector<uint32_t> list(1, 0u);   // [0] the count, then the tiles (128 to-rows x 64 from-rows) that hold a row of the caller's
    if (grid_wgs > 0) {
        const int ntx = RFpad / 64;
        for (int ty = 0; ty * 128 < nrt; ++ty)
            for (int tx = 0; tx * 64 < nrf; ++tx) list.push_back((uint32_t)(ty * ntx + tx));
        list[0] = (uint32_t)(list.size() - 1);
        if (int rc = d_list.reserve(list.size() * 4)) return rc;
        LDW_HIP(hipMemcpyAsync(d_list.p, list.data(), list.size() * 4, hipMemcpyHostToDevice, c->stream));
    }
    if (int rc = d_rl.reserve(rl.size() * 4)) return rc;
    if (int rc = d_pt.reserve((size_t)M2 * RTpad * 32)) return rc;
    if (int rc = d_pf.reserve((size_t)M2 * RFpad * 32)) return rc;
    if (int rc = d_G.reserve((size_t)RTpad * RFpad * 4)) return rc;
    LDW_HIP(hipMemcpyAsync(d_rl.p, rl.data(), rl.size() * 4, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemsetAsync(d_G.p, 0xFF, (size_t)RTpad * RFpad * 4, c->stream));   // (every entry must be WRITTEN by the kernel)
    if (int r2 = launch_pack_panel(c, d_rl.as<int32_t>() + RTpad, RFpad, d_pf.as<uint64_t>(), c->stream, d_rl.as<int32_t>(), RTpad, d_pt.as<uint64_t>())) return r2;
    ApxGemmArgs P;
    memset(&P, 0, sizeof(P));
    P.panel_t = d_pt.as<uint64_t>();
    P.panel_f = d_pf.as<uint64_t>();
    P.RTpad = RTpad;
    P.RFpad = RFpad;
    P.M2 = M2;
    P.dig_a = c->apx.dig_a.as<uint8_t>();
    P.dig_b = c->apx.dig_b.as<uint8_t>();
    P.shift = c->apx.apx_shift.as<int32_t>();
    P.G = d_G.as<int32_t>();
    P.fine = c->apx.apx_fine ? 1 : 0;
    if (grid_wgs > 0) {   // (no table fusion: every listed tile is stored)
        P.n_live = d_list.as<unsigned int>();
        P.tile_list = d_list.as<uint32_t>() + 1;
        P.grid_wgs = grid_wgs;
    }
    if (int r2 = launch_gemm_apx(c, P, c->stream)) return r2;
    std::vector<int32_t> h((size_t)RTpad * RFpad);
    LDW_HIP(hipMemcpyAsync(h.data(), d_G.p, h.size() * 4, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    for (int t = 0; t < nrt; ++t) memcpy(out + (size_t)t * nrf, h.data() + (size_t)t * RFpad, (size_t)nrf * 4);
    return LDW_OK;
}

static_assert(LDW_DEBUG_APX_MAYBE_MAX == APX_MAYBE_MAX, "ldweaver_amd_debug.h documents the build's APX_MAYBE_MAX");
static_assert(sizeof(ApxMaybe) == 12, "maybe_out is [maybe_cap][3] 32-bit words");

int ldw_debug_apx_gemm_fused(ldw_ctx *c, const int32_t *rows_t, int nrt, const int32_t *rows_f, int nrf, const uint8_t *bin_t, const uint8_t *bin_f, const uint8_t *rflag_t,
                             const uint8_t *rflag_f, const int32_t *tab, const uint8_t *sr_mask, int lower_only, int prune, int grid_wgs, int maybe_cap, int32_t *G_out,
                             uint8_t *clean_out, uint32_t *tiles_out, int32_t *maybe_out, int64_t counts_out[4]) {
    if (int rc = check_gpu(c)) return rc;
    if (int rc = join_prepare(c)) return rc;
    if (int rc = ensure_rows(c)) return rc;
    LDW_REQUIRE(rows_t && rows_f && bin_t && bin_f && tab && G_out && clean_out && counts_out && nrt > 0 && nrf > 0 && nrt <= 8192 && nrf <= 8192, LDW_ERR_ARG,
                "ldw_debug_apx_gemm_fused: bad argument");
    LDW_REQUIRE(c->apx.apx_ok, LDW_ERR_STATE, "ldw_debug_apx_gemm_fused: the weights do not allow the approximate path (%s)", c->apx.apx_gate.c_str());
    LDW_REQUIRE((rflag_t == nullptr) == (rflag_f == nullptr), LDW_ERR_ARG, "ldw_debug_apx_gemm_fused: the row flags of one side only");
    LDW_REQUIRE(prune ? (grid_wgs >= 0 && grid_wgs <= 65536) : grid_wgs == 0, LDW_ERR_ARG, "ldw_debug_apx_gemm_fused: grid of %d workgroups (prune %d: 0%s)", grid_wgs, prune,
                prune ? "..65536" : " only");
    LDW_REQUIRE(maybe_cap == -1 || (maybe_cap >= 1 && maybe_cap <= (1 << 20)), LDW_ERR_ARG, "ldw_debug_apx_gemm_fused: maybe list capacity %d outside -1, 1..1048576", maybe_cap);
    LDW_REQUIRE((!prune || tiles_out) && (maybe_cap < 0 || maybe_out), LDW_ERR_ARG, "ldw_debug_apx_gemm_fused: no room for the tile list or the maybe list");
    for (int k = 0; k < nrt; ++k) {
        LDW_REQUIRE(rows_t[k] >= 0 && rows_t[k] <= c->rows.R, LDW_ERR_ARG, "ldw_debug_apx_gemm_fused: to-side row %d = %d outside 0..R", k, rows_t[k]);
        LDW_REQUIRE(bin_t[k] < 64 || bin_t[k] == 255, LDW_ERR_ARG, "ldw_debug_apx_gemm_fused: to-side bin %d = %d", k, bin_t[k]);
    }
    for (int k = 0; k < nrf; ++k) {
        LDW_REQUIRE(rows_f[k] >= 0 && rows_f[k] <= c->rows.R, LDW_ERR_ARG, "ldw_debug_apx_gemm_fused: from-side row %d = %d outside 0..R", k, rows_f[k]);
        LDW_REQUIRE(bin_f[k] < 64 || bin_f[k] == 255, LDW_ERR_ARG, "ldw_debug_apx_gemm_fused: from-side bin %d = %d", k, bin_f[k]);
    }
    const int RTpad = (nrt + APX_TW - 1) / APX_TW * APX_TW, RFpad = (nrf + APX_TW - 1) / APX_TW * APX_TW, M2 = (int)(c->KW / 2);
    const size_t n_G = (size_t)RTpad * RFpad, n_clean = (size_t)(RTpad / 32) * (RFpad / 64), n_tiles = (size_t)(RTpad / 128) * (RFpad / 64);
    // the row lists, bins and flags as prep_block / k_build_packs leave them: padding -> the all-zero row R, no bin, no flag
    std::vector<int32_t> rl((size_t)RTpad + RFpad, (int32_t)c->rows.R);
    std::vector<uint8_t> bins((size_t)RTpad + RFpad, (uint8_t)255), flags((size_t)RTpad + RFpad, (uint8_t)0);
    std::copy(rows_t, rows_t + nrt, rl.begin());
    std::copy(rows_f, rows_f + nrf, rl.begin() + RTpad);
    std::copy(bin_t, bin_t + nrt, bins.begin());
    std::copy(bin_f, bin_f + nrf, bins.begin() + RTpad);
    if (rflag_t) {
        std::copy(rflag_t, rflag_t + nrt, flags.begin());
        std::copy(rflag_f, rflag_f + nrf, flags.begin() + RTpad);
    }
    DevBuf d_rl, d_pt, d_pf, d_G, d_bins, d_flags, d_tab, d_mask, d_clean, d_list, d_ctr, d_maybe;
    auto up = [&](DevBuf &b, const void *src, size_t bytes) -> int {
        if (int rc = b.reserve(bytes)) return rc;
        LDW_HIP(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
        return LDW_OK;
    };
    auto filled = [&](DevBuf &b, size_t bytes) -> int {
        if (int rc = b.reserve(bytes)) return rc;
        LDW_HIP(hipMemsetAsync(b.p, LDW_DEBUG_APX_FUSED_FILL, bytes, c->stream));
        return LDW_OK;
    };
    if (int rc = up(d_rl, rl.data(), rl.size() * 4)) return rc;
    if (int rc = up(d_bins, bins.data(), bins.size())) return rc;
    if (int rc = up(d_flags, flags.data(), flags.size())) return rc;
    if (int rc = up(d_tab, tab, (size_t)64 * 64 * 8)) return rc;
    if (sr_mask)
        if (int rc = up(d_mask, sr_mask, n_tiles)) return rc;
    if (int rc = d_pt.reserve((size_t)M2 * RTpad * 32)) return rc;
    if (int rc = d_pf.reserve((size_t)M2 * RFpad * 32)) return rc;
    if (int rc = filled(d_G, n_G * 4)) return rc;
    if (int rc = filled(d_clean, n_clean)) return rc;
    if (int rc = filled(d_list, n_tiles * 4)) return rc;
    constexpr int MAYBE_GUARD = 64;   // entries behind the capacity: they must keep the fill (counts_out[3])
    if (maybe_cap > 0)
        if (int rc = filled(d_maybe, ((size_t)maybe_cap + MAYBE_GUARD) * sizeof(ApxMaybe))) return rc;
    // the three counters the launches add to, zeroed as the product zeroes them: [0] skipped tiles (64 bits), [2] live tiles, [3] maybe entries
    if (int rc = d_ctr.reserve(64)) return rc;
    LDW_HIP(hipMemsetAsync(d_ctr.p, 0, 64, c->stream));
    if (int r2 = launch_pack_panel(c, d_rl.as<int32_t>() + RTpad, RFpad, d_pf.as<uint64_t>(), c->stream, d_rl.as<int32_t>(), RTpad, d_pt.as<uint64_t>())) return r2;
    ApxGemmArgs P;
    memset(&P, 0, sizeof(P));
    P.panel_t = d_pt.as<uint64_t>();
    P.panel_f = d_pf.as<uint64_t>();
    P.RTpad = RTpad;
    P.RFpad = RFpad;
    P.M2 = M2;
    P.dig_a = c->apx.dig_a.as<uint8_t>();
    P.dig_b = c->apx.dig_b.as<uint8_t>();
    P.shift = c->apx.apx_shift.as<int32_t>();
    P.fine = c->apx.apx_fine ? 1 : 0;
    P.G = d_G.as<int32_t>();
    P.lower_only = lower_only ? 1 : 0;
    P.fuse = 1;
    if (prune) {   // (as the block's launch chain fills them, ldw_mi_block.inc: the row flags go with the live-tile pass only)
        P.skip_ctr = d_ctr.as<unsigned long long>();
        P.tile_list = d_list.as<uint32_t>();
        P.n_live = d_ctr.as<unsigned int>() + 2;
        P.grid_wgs = grid_wgs > 0 ? grid_wgs : apx_run_grid(c, RTpad, RFpad);
        if (rflag_t) {
            P.rflag_t = d_flags.as<uint8_t>();
            P.rflag_f = d_flags.as<uint8_t>() + RTpad;
        }
    }
    P.bin_t = d_bins.as<uint8_t>();
    P.bin_f = d_bins.as<uint8_t>() + RTpad;
    P.tab = d_tab.as<int2>();
    P.tab_nb = 64;
    P.clean = d_clean.as<uint8_t>();
    P.sr_mask = sr_mask ? d_mask.as<uint8_t>() : nullptr;
    if (maybe_cap > 0) {
        P.maybe = d_maybe.as<ApxMaybe>();
        P.maybe_n = d_ctr.as<unsigned int>() + 3;
        P.maybe_cap = (unsigned int)maybe_cap;
    }
    // the hook is no block of a pass: what the launch code adds to the context's counters is taken off again (ldw_gemm_stats, ldw_prune_report)
    double stat[6];
    memcpy(stat, c->cnt.gemm_stat, sizeof(stat));
    const int64_t waves_total = c->cnt.apx_waves_total;
    const double ops_per_wave = c->apx_ops_per_wave;
    int rc = prune ? launch_apx_live_tiles(c, P, c->stream) : LDW_OK;
    if (rc == LDW_OK) rc = launch_gemm_apx(c, P, c->stream);
    memcpy(c->cnt.gemm_stat, stat, sizeof(stat));
    c->cnt.apx_waves_total = waves_total;
    c->apx_ops_per_wave = ops_per_wave;
    uint32_t ctr[4] = {0u, 0u, 0u, 0u};
    std::vector<uint8_t> guard(maybe_cap > 0 ? MAYBE_GUARD * sizeof(ApxMaybe) : 0, (uint8_t)LDW_DEBUG_APX_FUSED_FILL);
    if (rc == LDW_OK) {
        LDW_HIP(hipMemcpyAsync(G_out, d_G.p, n_G * 4, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipMemcpyAsync(clean_out, d_clean.p, n_clean, hipMemcpyDeviceToHost, c->stream));
        if (tiles_out) LDW_HIP(hipMemcpyAsync(tiles_out, d_list.p, n_tiles * 4, hipMemcpyDeviceToHost, c->stream));
        if (maybe_cap > 0) {
            LDW_HIP(hipMemcpyAsync(maybe_out, d_maybe.p, (size_t)maybe_cap * sizeof(ApxMaybe), hipMemcpyDeviceToHost, c->stream));
            LDW_HIP(hipMemcpyAsync(guard.data(), d_maybe.as<ApxMaybe>() + maybe_cap, guard.size(), hipMemcpyDeviceToHost, c->stream));
        }
        LDW_HIP(hipMemcpyAsync(ctr, d_ctr.p, sizeof(ctr), hipMemcpyDeviceToHost, c->stream));
    }
    LDW_HIP(hipStreamSynchronize(c->stream));   // (the uploads read this frame)
    if (rc != LDW_OK) return rc;
    counts_out[0] = ctr[2];
    counts_out[1] = (int64_t)(((uint64_t)ctr[1] << 32) | ctr[0]);
    counts_out[2] = ctr[3];
    counts_out[3] = (int64_t)std::count_if(guard.begin(), guard.end(), [](uint8_t b) { return b != (uint8_t)LDW_DEBUG_APX_FUSED_FILL; });
    return LDW_OK;
}

int ldw_debug_limb_gemm(ldw_ctx *c, int engine, const int32_t *rows_t, int nrt, const int32_t *rows_f, int nrf, int limb0, int nlimbs, int lower_only, int by0, int by1,
                        const uint8_t *tile_mask, const uint32_t *tile_list, int n_tile_list, int64_t *out) {
    if (int rc = check_gpu(c)) return rc;
    if (int rc = join_prepare(c)) return rc;
    LDW_REQUIRE(engine == 0 || engine == 1, LDW_ERR_ARG, "ldw_debug_limb_gemm: engine %d outside 0..1", engine);
    LDW_REQUIRE(rows_t && rows_f && out && nrt > 0 && nrf > 0 && nrt <= 8192 && nrf <= 8192, LDW_ERR_ARG, "ldw_debug_limb_gemm: bad argument");
    LDW_REQUIRE(c->wts.have_weights && c->wts.digits.p, LDW_ERR_STATE, "ldw_debug_limb_gemm: no weights (ldw_set_weights)");
    if (int rc = ensure_rows(c)) return rc;
    for (int k = 0; k < nrt; ++k) LDW_REQUIRE(rows_t[k] >= 0 && rows_t[k] <= c->rows.R, LDW_ERR_ARG, "ldw_debug_limb_gemm: to-side row %d = %d outside 0..R", k, rows_t[k]);
    for (int k = 0; k < nrf; ++k) LDW_REQUIRE(rows_f[k] >= 0 && rows_f[k] <= c->rows.R, LDW_ERR_ARG, "ldw_debug_limb_gemm: from-side row %d = %d outside 0..R", k, rows_f[k]);
    const int RTpad = (nrt + TILE - 1) / TILE * TILE, RFpad = (nrf + TILE - 1) / TILE * TILE, nby = RTpad / TILE, nbx = RFpad / TILE_F4;
    // everything the launch code would refuse, and what it trusts (the tiles of a list), before anything is queued
    LDW_REQUIRE(nlimbs >= 1 && nlimbs <= 6, LDW_ERR_ARG, "ldw_debug_limb_gemm: nlimbs %d outside 1..6", nlimbs);
    LDW_REQUIRE(limb0 >= 0 && limb0 + nlimbs <= c->wts.nlimbs, LDW_ERR_ARG, "ldw_debug_limb_gemm: limbs %d..%d beyond the %d of the weights", limb0, limb0 + nlimbs - 1, c->wts.nlimbs);
    const int by_end = by1 < 0 ? nby : by1;
    LDW_REQUIRE(by0 >= 0 && by0 < by_end && by_end <= nby, LDW_ERR_ARG, "ldw_debug_limb_gemm: bad tile-row range %d..%d of %d", by0, by1, nby);
    LDW_REQUIRE(tile_list || n_tile_list == 0, LDW_ERR_ARG, "ldw_debug_limb_gemm: %d listed tiles without a list", n_tile_list);
    if (tile_list) {
        LDW_REQUIRE(n_tile_list >= 0 && n_tile_list <= 65536 && by0 == 0, LDW_ERR_ARG, "ldw_debug_limb_gemm: bad tile list (%d entries, by0 %d)", n_tile_list, by0);
        for (int k = 0; k < n_tile_list; ++k)
            LDW_REQUIRE((int)(tile_list[k] >> 16) < nby && (int)(tile_list[k] & 0xFFFFu) < nbx, LDW_ERR_ARG, "ldw_debug_limb_gemm: listed tile %d = (%u, %u) outside the %d x %d grid", k,
                        tile_list[k] >> 16, tile_list[k] & 0xFFFFu, nby, nbx);
    }
    if (engine == 1) {
        LDW_REQUIRE(limb0 == 0 && nlimbs == c->wts.nlimbs && !tile_mask && !tile_list && by0 == 0 && by_end == nby, LDW_ERR_ARG,
                    "ldw_debug_limb_gemm: the popcount engine takes all limbs, no mask, no list and no strip");
        LDW_REQUIRE(c->N <= 65535, LDW_ERR_ARG, "ldw_debug_limb_gemm: the popcount engine holds at most 65535 sequences (%lld)", (long long)c->N);
        LDW_REQUIRE(c->apx.pop_segs.p && c->apx.pop_wbeg.p, LDW_ERR_STATE, "ldw_debug_limb_gemm: no popcount segments (ldw_set_weights)");
    }
    std::vector<int32_t> rl((size_t)RTpad + RFpad, (int32_t)c->rows.R);   // padding -> the all-zero row R
    std::copy(rows_t, rows_t + nrt, rl.begin());
    std::copy(rows_f, rows_f + nrf, rl.begin() + RTpad);
    const size_t n_out = (size_t)RTpad * RFpad, n_mask = (size_t)nby * nbx;
    DevBuf d_rl, d_G, d_mask, d_list;
    if (int rc = d_rl.reserve(rl.size() * 4)) return rc;
    if (int rc = d_G.reserve(n_out * 8)) return rc;
    LDW_HIP(hipMemcpyAsync(d_rl.p, rl.data(), rl.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (tile_mask) {
        if (int rc = d_mask.reserve(n_mask)) return rc;
        LDW_HIP(hipMemcpyAsync(d_mask.p, tile_mask, n_mask, hipMemcpyHostToDevice, c->stream));
    }
    if (tile_list) {
        if (int rc = d_list.reserve((size_t)std::max(1, n_tile_list) * 4)) return rc;
        if (n_tile_list > 0) LDW_HIP(hipMemcpyAsync(d_list.p, tile_list, (size_t)n_tile_list * 4, hipMemcpyHostToDevice, c->stream));
    }
    LDW_HIP(hipMemsetAsync(d_G.p, LDW_DEBUG_LIMB_GEMM_FILL, n_out * 8, c->stream));   // (an entry no kernel wrote shows)
    double stat[6];
    memcpy(stat, c->cnt.gemm_stat, sizeof(stat));   // the hook is no block-wide GEMM of a pass: ldw_gemm_stats does not see it
    int rc;
    if (engine == 1) rc = launch_cooc_popc(c, d_rl.as<int32_t>(), RTpad, d_rl.as<int32_t>() + RTpad, RFpad, d_G.as<int64_t>(), lower_only, c->stream);
    else
        rc = launch_gemm_bits(c, c->rows.Mbits.as<uint64_t>(), c->KW, d_rl.as<int32_t>(), RTpad, d_rl.as<int32_t>() + RTpad, RFpad, d_G.as<int64_t>(), nlimbs,
                              c->wts.digits.as<int8_t>() + (int64_t)limb0 * c->KW * 64, lower_only, c->stream, by0, by1, tile_mask ? d_mask.as<uint8_t>() : nullptr,
                              tile_list ? d_list.as<uint32_t>() : nullptr, n_tile_list);
    memcpy(c->cnt.gemm_stat, stat, sizeof(stat));
    std::vector<int64_t> h;
    if (rc == LDW_OK) {
        h.resize(n_out);
        LDW_HIP(hipMemcpyAsync(h.data(), d_G.p, n_out * 8, hipMemcpyDeviceToHost, c->stream));
    }
    LDW_HIP(hipStreamSynchronize(c->stream));   // (the uploads read this frame)
    if (rc != LDW_OK) return rc;
    for (int t = 0; t < nrt; ++t) memcpy(out + (size_t)t * nrf, h.data() + (size_t)t * RFpad, (size_t)nrf * 8);
    return LDW_OK;
}

int ldw_debug_lo_units(ldw_ctx *c, const int32_t *from_snps, int ntiles, const int32_t *to_snps, int nt, const uint32_t *counts, const int32_t *slots, int32_t geom_out[8],
                       int32_t *cmax_out, int64_t *tile_base_out, int64_t *glo_total_out, int32_t *glo_out, int64_t glo_capacity) {
    if (int rc = check_gpu(c)) return rc;
    if (int rc = join_prepare(c)) return rc;
    LDW_REQUIRE(from_snps && to_snps && counts && slots && geom_out && cmax_out && tile_base_out && glo_total_out, LDW_ERR_ARG, "ldw_debug_lo_units: null argument");
    LDW_REQUIRE(ntiles >= 1 && ntiles <= 4096 && nt >= 1 && nt <= (1 << 20), LDW_ERR_ARG, "ldw_debug_lo_units: %d from-tiles (1..4096) or %d to-side SNPs (1..1048576)", ntiles, nt);
    LDW_REQUIRE(c->wts.have_weights && c->wts.digits.p, LDW_ERR_STATE, "ldw_debug_lo_units: no weights (ldw_set_weights)");
    LDW_REQUIRE(c->wts.nlimbs >= 2, LDW_ERR_STATE, "ldw_debug_lo_units: the weights have %d limb, the low-limb GEMM reads two", c->wts.nlimbs);
    if (int rc = ensure_rows(c)) return rc;
    const std::vector<int32_t> &row0 = c->rows.h_row0;
    for (int k = 0; k < 64 * ntiles; ++k) LDW_REQUIRE(from_snps[k] >= -1 && from_snps[k] < c->L, LDW_ERR_ARG, "ldw_debug_lo_units: from-side lane %d = %d outside -1..L-1", k, from_snps[k]);
    for (int k = 0; k < nt; ++k) LDW_REQUIRE(to_snps[k] >= 0 && to_snps[k] < c->L, LDW_ERR_ARG, "ldw_debug_lo_units: to-side SNP %d = %d outside 0..L-1", k, to_snps[k]);
    auto rows_of = [&](int32_t snp) { return (int)(row0[(size_t)snp + 1] - row0[(size_t)snp]); };
    std::vector<int32_t> cmax, tf;
    std::vector<int64_t> tbase;
    const LoLayout g = lo_layout(
        nt, [&](int64_t k) { return rows_of(to_snps[k]); }, (size_t)64 * ntiles, [&](size_t t) { return from_snps[t] < 0 ? -1 : rows_of(from_snps[t]); }, cmax, tbase, tf);
    LDW_REQUIRE(g.n_tf > 0 && g.n_tf <= 65535 && g.glo_total > 0 && g.glo_total <= ((int64_t)1 << 28), LDW_ERR_ARG, "ldw_debug_lo_units: %d (tile, fs) pairs or %lld ints of sums beyond the hook's limits",
                g.n_tf, (long long)g.glo_total);
    // the unit lists as k_mi_screen leaves them: tl[tile * nt + uoff[lc] + k] = the column slot
    std::vector<uint32_t> tl((size_t)ntiles * nt, 0u), cnt((size_t)ntiles * 3);
    size_t at = 0;
    for (int t = 0; t < ntiles; ++t)
        for (int lc = 0; lc < 3; ++lc) {
            const uint32_t n = counts[t * 3 + lc];
            LDW_REQUIRE(n <= (uint32_t)g.n_lc[lc], LDW_ERR_ARG, "ldw_debug_lo_units: tile %d lists %u units of class %d, the to side holds %d", t, n, lc, g.n_lc[lc]);
            cnt[(size_t)t * 3 + lc] = n;
            for (uint32_t k = 0; k < n; ++k, ++at) {
                const int32_t q = slots[at];
                LDW_REQUIRE(q >= 0 && q < nt && lo_class(rows_of(to_snps[q])) == lc, LDW_ERR_ARG, "ldw_debug_lo_units: tile %d class %d unit %u: slot %d outside 0..nt-1 or of another class", t, lc,
                            k, q);
                tl[(size_t)t * nt + g.uoff[lc] + k] = (uint32_t)q;
            }
        }
    for (int k = 0; k < 3; ++k) {
        geom_out[k] = g.rowbase[k];
        geom_out[3 + k] = g.uoff[k];
    }
    geom_out[6] = g.RTlo;
    geom_out[7] = g.n_tf;
    std::copy(cmax.begin(), cmax.end(), cmax_out);
    std::copy(tbase.begin(), tbase.end(), tile_base_out);
    *glo_total_out = g.glo_total;
    if (!glo_out) return LDW_OK;
    LDW_REQUIRE(glo_capacity >= g.glo_total, LDW_ERR_SIZE, "ldw_debug_lo_units: capacity %lld < %lld ints", (long long)glo_capacity, (long long)g.glo_total);
    std::vector<int32_t> idx_f((size_t)c->L), perm_t((size_t)nt);   // from side: the lanes name their SNPs; to side: slot q is entry q
    for (int64_t k = 0; k < c->L; ++k) idx_f[(size_t)k] = (int32_t)k;
    for (int k = 0; k < nt; ++k) perm_t[(size_t)k] = k;
    DevBuf d_pf, d_if, d_pt, d_it, d_cmax, d_tb, d_tf, d_cnt, d_tl, d_glo;
    auto up = [&](DevBuf &b, const void *src, size_t bytes) -> int {
        if (int rc = b.reserve(bytes)) return rc;
        LDW_HIP(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
        return LDW_OK;
    };
    if (int rc = up(d_pf, from_snps, (size_t)64 * ntiles * 4)) return rc;
    if (int rc = up(d_if, idx_f.data(), idx_f.size() * 4)) return rc;
    if (int rc = up(d_pt, perm_t.data(), perm_t.size() * 4)) return rc;
    if (int rc = up(d_it, to_snps, (size_t)nt * 4)) return rc;
    if (int rc = up(d_cmax, cmax.data(), cmax.size() * 4)) return rc;
    if (int rc = up(d_tb, tbase.data(), tbase.size() * 8)) return rc;
    if (int rc = up(d_tf, tf.data(), tf.size() * 4)) return rc;
    if (int rc = up(d_cnt, cnt.data(), cnt.size() * 4)) return rc;
    if (int rc = up(d_tl, tl.data(), tl.size() * 4)) return rc;
    if (int rc = d_glo.reserve((size_t)g.glo_total * 4 + 64)) return rc;
    LDW_HIP(hipMemsetAsync(d_glo.p, LDW_DEBUG_LO_UNITS_FILL, (size_t)g.glo_total * 4, c->stream));
    LoGemmArgs P;
    memset(&P, 0, sizeof(P));
    P.Mbits = c->rows.Mbits.as<uint64_t>();
    P.KW = c->KW;
    P.Kpad = c->KW * 64;
    P.digits_lo = c->wts.digits.as<int8_t>();
    P.perm_f = d_pf.as<int32_t>();
    P.idx_f = d_if.as<int32_t>();
    P.perm_t = d_pt.as<int32_t>();
    P.idx_t = d_it.as<int32_t>();
    P.row0 = c->rows.row0.as<int32_t>();
    P.zero_row = (int32_t)c->rows.R;
    P.nf = 64 * ntiles;
    P.nt = nt;
    P.tf_list = d_tf.as<int32_t>();
    for (int k = 0; k < 3; ++k) {
        P.lo.n_lc[k] = g.n_lc[k];
        P.lo.uoff[k] = g.uoff[k];
        P.lo.rowbase[k] = g.rowbase[k];
    }
    P.lo.RTlo = g.RTlo;
    P.lo.ntiles = g.ntiles;
    P.lo.on = 1;
    P.lo.cmax_f = d_cmax.as<int32_t>();
    P.lo.tile_base = d_tb.as<int64_t>();
    P.lo.cnt = d_cnt.as<unsigned int>();
    P.lo.tl = d_tl.as<uint32_t>();
    P.lo.glo = d_glo.as<int32_t>();
    const int rc = launch_gemm_lo_units(c, P, g.n_tf, c->stream);
    if (rc == LDW_OK) LDW_HIP(hipMemcpyAsync(glo_out, d_glo.p, (size_t)g.glo_total * 4, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));   // (the uploads read this frame)
    return rc;
}

int ldw_debug_pair_sums(ldw_ctx *c, int form, int grid_wgs, uint32_t cap, const uint32_t *counts, const int32_t *snp_a, const int32_t *snp_b, int64_t *sums_out,
                        int *form_out) {
    if (int rc = check_gpu(c)) return rc;
    if (int rc = join_prepare(c)) return rc;
    LDW_REQUIRE(counts && snp_a && snp_b && sums_out, LDW_ERR_ARG, "ldw_debug_pair_sums: null argument");
    LDW_REQUIRE(cap >= 1 && cap <= 65536, LDW_ERR_ARG, "ldw_debug_pair_sums: list capacity %u outside 1..65536", cap);
    LDW_REQUIRE(form >= 0 && form <= 4, LDW_ERR_ARG, "ldw_debug_pair_sums: form %d outside 0..4", form);
    LDW_REQUIRE(grid_wgs >= 0 && grid_wgs <= 65536, LDW_ERR_ARG, "ldw_debug_pair_sums: grid of %d workgroups outside 0..65536", grid_wgs);
    LDW_REQUIRE(c->wts.have_weights && c->apx.pop_segs.p && c->apx.pop_wbeg.p, LDW_ERR_STATE, "ldw_debug_pair_sums: the weight tables of the approximate path are not prepared (ldw_set_weights)");
    if (int rc = ensure_rows(c)) return rc;
    constexpr int NL = PAIR_PATHS * PAIR_SHARDS;
    static const int path_na[4] = {1, 2, 1, 2}, path_nb[4] = {1, 1, 2, 2};
    // the entries as flush_pairs (ldw_mi_screen.inc) writes them: first bit row | row count << 29 of both SNPs
    std::vector<PairEnt> ents((size_t)NL * cap, PairEnt{0u, 0u, 0u, 0u});
    for (int sub = 0; sub < NL; ++sub) {
        const int path = sub / PAIR_SHARDS;
        const uint32_t n = std::min(counts[sub], cap);
        for (uint32_t k = 0; k < n; ++k) {
            const size_t at = (size_t)sub * cap + k;
            const int64_t a = snp_a[at], b = snp_b[at];
            LDW_REQUIRE(a >= 0 && a < c->L && b >= 0 && b < c->L, LDW_ERR_ARG, "ldw_debug_pair_sums: list %d entry %u: SNPs (%lld, %lld) outside 0..L-1", sub, k, (long long)a,
                        (long long)b);
            const int32_t r0a = c->rows.h_row0[(size_t)a], r0b = c->rows.h_row0[(size_t)b];
            const int na = c->rows.h_row0[(size_t)a + 1] - r0a, nb = c->rows.h_row0[(size_t)b + 1] - r0b;
            if (path < 4) LDW_REQUIRE(na == path_na[path] && nb == path_nb[path], LDW_ERR_ARG, "ldw_debug_pair_sums: list %d entry %u: %d x %d rows in the list of %d x %d", sub, k, na, nb, path_na[path], path_nb[path]);
            else LDW_REQUIRE(na >= 1 && na <= 4 && nb >= 1 && nb <= 4, LDW_ERR_ARG, "ldw_debug_pair_sums: list %d entry %u: %d x %d rows outside 1..4", sub, k, na, nb);
            ents[at] = PairEnt{k, k, (uint32_t)r0a | ((uint32_t)na << 29), (uint32_t)r0b | ((uint32_t)nb << 29)};
        }
    }
    const size_t n_sums = (size_t)NL * cap * 16;
    DevBuf d_n, d_ents, d_sums;
    if (int rc = d_n.reserve(NL * 4)) return rc;
    if (int rc = d_ents.reserve(ents.size() * sizeof(PairEnt))) return rc;
    if (int rc = d_sums.reserve(n_sums * 8)) return rc;
    LDW_HIP(hipMemcpyAsync(d_n.p, counts, NL * 4, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(d_ents.p, ents.data(), ents.size() * sizeof(PairEnt), hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemsetAsync(d_sums.p, LDW_DEBUG_PAIR_SUMS_FILL, n_sums * 8, c->stream));   // (a store outside the entries k_pair_mi reads shows)
    EpiArgs A;
    memset(&A, 0, sizeof(A));
    A.pl_n = d_n.as<unsigned int>();
    A.pl_pairs = d_ents.as<PairEnt>();
    A.pl_cap = cap;
    PairSumsRan ran;
    const int rc = launch_pair_sums(c, A, d_sums.as<int64_t>(), c->stream, form, grid_wgs, &ran);
    if (rc == LDW_OK) {
        LDW_HIP(hipGetLastError());
        LDW_HIP(hipMemcpyAsync(sums_out, d_sums.p, n_sums * 8, hipMemcpyDeviceToHost, c->stream));
    }
    LDW_HIP(hipStreamSynchronize(c->stream));   // (the uploads read this frame)
    if (rc == LDW_OK && form_out) *form_out = ran.form;
    return rc;
}

int ldw_debug_screen_bound(ldw_ctx *c, int kind, int na, int nb, int64_t n, const int64_t *g, const int64_t *pa, const int64_t *pb, const float *pX, const float *pY,
                           const double *rr, const uint32_t *masks, const double params[20], float *out, double *out64) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(n > 0 && n < ((int64_t)1 << 28) && g && pa && pb && pX && pY && rr && params, LDW_ERR_ARG, "ldw_debug_screen_bound: bad argument");
    LDW_REQUIRE(kind >= 0 && kind <= 4 && ((kind == 4) ? out64 != nullptr : out != nullptr), LDW_ERR_ARG, "ldw_debug_screen_bound: kind %d / missing output", kind);
    const bool generic = kind == 1 || kind == 3;
    LDW_REQUIRE(generic ? masks != nullptr : ((na == 1 || na == 2) && (nb == 1 || nb == 2)), LDW_ERR_ARG, "ldw_debug_screen_bound: kinds 0 / 2 / 4 take na, nb in {1, 2}; kinds 1 / 3 take masks");
    const bool apx = kind == 0 || kind == 1;
    std::vector<int32_t> g32;
    if (apx) {
        g32.resize((size_t)n * 16);
        for (size_t k = 0; k < g32.size(); ++k) {
            LDW_REQUIRE(g[k] >= -2147483647LL && g[k] <= 2147483647LL, LDW_ERR_ARG, "ldw_debug_screen_bound: entry %zu does not fit int32", k);
            g32[k] = (int32_t)g[k];
        }
    }
    DevBuf B;
    const size_t sz_g = (size_t)n * 16 * 8, sz_g32 = (size_t)n * 16 * 4, sz_p = (size_t)n * 5 * 8, sz_f = (size_t)n * 5 * 4, sz_r = (size_t)n * 3 * 8, sz_m = (size_t)n * 2 * 4,
                 sz_o = (size_t)n * 4, sz_o64 = (size_t)n * 8;
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t o_g = 0, o_g32 = o_g + al(sz_g), o_pa = o_g32 + al(sz_g32), o_pb = o_pa + al(sz_p), o_pX = o_pb + al(sz_p), o_pY = o_pX + al(sz_f), o_rr = o_pY + al(sz_f),
                 o_m = o_rr + al(sz_r), o_o = o_m + al(sz_m), o_o64 = o_o + al(sz_o), total = o_o64 + al(sz_o64);
    if (int rc = B.reserve(total)) return rc;
    char *base = B.as<char>();
    LDW_HIP(hipMemcpyAsync(base + o_g, g, sz_g, hipMemcpyHostToDevice, c->stream));
    if (apx) LDW_HIP(hipMemcpyAsync(base + o_g32, g32.data(), sz_g32, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(base + o_pa, pa, sz_p, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(base + o_pb, pb, sz_p, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(base + o_pX, pX, sz_f, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(base + o_pY, pY, sz_f, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(base + o_rr, rr, sz_r, hipMemcpyHostToDevice, c->stream));
    if (masks) LDW_HIP(hipMemcpyAsync(base + o_m, masks, sz_m, hipMemcpyHostToDevice, c->stream));
    EpiArgs A;
    memset(&A, 0, sizeof(A));
    A.neff = params[5];
    A.scale = std::ldexp(1.0, -(int)params[0]);
    A.quirk = LDW_QUIRK_INTENDED;
    A.E.apx = apx ? 1 : 0;
    A.E.apx_EG = (float)params[6];
    A.E.apx_dfac = (float)params[7];
    A.E.apx_s1 = (float)params[8];
    A.E.apx_c1 = (float)params[9];
    A.E.apx_W = params[10];
    A.E.apx_unit = params[11];
    A.E.apx_MU = (float)params[18];
    A.E.scr_shift = apx ? 0 : (int)params[13];
    A.E.scr_scale = (float)(apx ? params[12] : params[14]);
    DbgArrays D;
    D.g = reinterpret_cast<const int64_t *>(base + o_g);
    D.g32 = reinterpret_cast<const int32_t *>(base + o_g32);
    D.pa = reinterpret_cast<const int64_t *>(base + o_pa);
    D.pb = reinterpret_cast<const int64_t *>(base + o_pb);
    D.pX = reinterpret_cast<const float *>(base + o_pX);
    D.pY = reinterpret_cast<const float *>(base + o_pY);
    D.rr = reinterpret_cast<const double *>(base + o_rr);
    D.mk = reinterpret_cast<const uint32_t *>(base + o_m);
    D.out = reinterpret_cast<float *>(base + o_o);
    D.out64 = reinterpret_cast<double *>(base + o_o64);
    D.n = n;
    const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
#define LDW_DBG_FULL(K)                                                                                   \
    {                                                                                                     \
        if (na == 1 && nb == 1) hipLaunchKernelGGL((k_dbg_full<1, 1, K>), grid, blk, 0, c->stream, A, D); \
        else if (na == 1) hipLaunchKernelGGL((k_dbg_full<1, 2, K>), grid, blk, 0, c->stream, A, D);       \
        else if (nb == 1) hipLaunchKernelGGL((k_dbg_full<2, 1, K>), grid, blk, 0, c->stream, A, D);       \
        else hipLaunchKernelGGL((k_dbg_full<2, 2, K>), grid, blk, 0, c->stream, A, D);                    \
    }
    if (kind == 0) LDW_DBG_FULL(0)
    else if (kind == 2) LDW_DBG_FULL(2)
    else if (kind == 4) LDW_DBG_FULL(4)
    else if (kind == 1) hipLaunchKernelGGL(k_dbg_generic<true>, grid, blk, 0, c->stream, A, D);
    else hipLaunchKernelGGL(k_dbg_generic<false>, grid, blk, 0, c->stream, A, D);
#undef LDW_DBG_FULL
    LDW_HIP(hipGetLastError());
    if (kind == 4) LDW_HIP(hipMemcpyAsync(out64, base + o_o64, sz_o64, hipMemcpyDeviceToHost, c->stream));
    else LDW_HIP(hipMemcpyAsync(out, base + o_o, sz_o, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    return LDW_OK;
}

}  // extern "C"
