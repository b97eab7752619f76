// MI epilogue, link selection and the block drivers (twins of perform_MI_computation_ACGTN,
// R/computePairwiseMI.R:167-386, and of the block loop of perform_MI_computation, :103-116).
//
// First block of a call sequence (no histogram-bucket guess yet), speculation misses, ldw_mi_block:
//   GEMM, 5 limbs (ldw_gemm_bits.hip) -> k_mi_epilogue_fast / _rest (ldw_mi_eval.inc): one thread per SNP pair turns the fixed-point joint sums into MI
//   (src/computeMI.cpp:19), writes the dense MI block, scatters the short-range links straight to their final rows and
//   histograms the long-range MI values in LDS -> k_pick_bucket: ranks of the two order statistics of quantile type 7
//   and the histogram bucket holding them -> k_lr_gather: every long-range pair at or above that bucket.
// Every other block (speculative: the guess is an earlier same-kind block's bucket minus an adaptive margin), DEFAULT path when the
// weights allow it (launch_block_apx, ldw_apx.hip): k_pack_panel -> k_zero4 -> k_build_packs -> gemm_apx_kernel (ONE dual-digit int8
//   pass into the int32 block G'; on off-diagonal blocks its epilogue applies the threshold table and neither stores nor flags for
//   screening the regions that pass) -> k_mi_screen<RM, true> / k_mi_screen_generic<true> (rigorous fp32 upper bound of MI from G';
//   long-range candidates go to PAIR lists, units with a short-range pair to the unit list) -> k_pair_sums / k_pair_mi (exact int64
//   sums of the listed pairs by class-wise popcounts, fp64 MI) + gemm_bits_kernel<5> on the band's tiles -> k_mi_units (short-range
//   units) -> k_pick_bucket.
// The limb paths (ldw_set_path(1), or weights the approximation cannot serve):
//   GEMM, 3 high limbs -> k_build_packs (per-block SNP constants in epilogue order) -> k_mi_screen / k_mi_screen_generic
//   (fp32 upper bound of MI per pair; lists the units = 64 from-side SNPs x 1 to-side SNP that hold a short-range pair
//   or a pair that may reach the guessed bucket) -> gemm_lo_units_kernel (the 2 low limbs of the listed units' joint sums)
//   -> k_mi_units<true|false> (fp64 MI of the listed units, short-range rows to their final rows, candidates >= the
//   guessed bucket appended and counted) -> k_pick_bucket (verifies the guess).
// Then, either way: k_sel_thresh / k_sel_mark / k_sel_scatter / k_sel_clear (radix select of the threshold, bitmap ranks: no sort), or,
// for blocks without a guess and very large candidate sets, two radix sorts (by MI, then by reference row order) with k_lr_thresh in
// between -> k_lr_append.
// The short-range test needs no arithmetic per pair: POS is ascending, so the partners of a to-side SNP within sr_dist
// (circularly) are at most three index intervals of the from-side list, found on the host by binary search (ColInfo).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include "ldw_prim.h"

#include "ldw_internal.h"
#include "ldw_dev.h"
#ifndef LDW_SCREEN_V
#define LDW_SCREEN_V 2   // columns in flight per wave in the multi-cell screen (tuning: make CXXFLAGS+=-DLDW_SCREEN_V=4)
#endif
#ifndef LDW_SCREEN_WAVES
#define LDW_SCREEN_WAVES 6   // waves per SIMD the screen is compiled for (80 VGPRs; 5: 96)
#endif
#include "ldw_epi.h"
#include "ldw_pass_plan.h"
#include <future>

#include "ldw_apx.h"
#include "ldw_pairs.h"

using namespace ldw;

namespace ldw {
#include "ldw_mi_screen.inc"
#include "ldw_mi_eval.inc"
#include "ldw_mi_select.inc"
}  // namespace ldw

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
namespace {
#include "ldw_mi_block.inc"
#include "ldw_mi_items.inc"
#include "ldw_mi_pass.inc"
}  // namespace

namespace ldw {
// Every creation is an idempotent ensure, and "ready" is set after the last one: a call that failed half-way is simply repeated.
int ensure_streams(ldw_ctx *c) {
    if (c->streams_ready) return LDW_OK;
    const unsigned quiet = hipEventDisableTiming;
    LDW_HIP(c->copy_stream.ensure(hipStreamNonBlocking));
    for (int k = 0; k < LDW_NSLOT; ++k) {
        LDW_HIP(c->ev_up[k].ensure(quiet));
        LDW_HIP(c->ev_done[k].ensure(quiet));
        LDW_HIP(c->ev_pick[k].ensure(quiet));
        LDW_HIP(c->ev_gemm[k].ensure(quiet));
        if (int rc = c->pin_pick[k].reserve((size_t)LDW_SPAN_MAX * PICK_STRIDE + 64, "ensure_streams")) return rc;
    }
    LDW_HIP(c->ev_lrc.ensure(quiet));
    for (auto &e : c->ev_probe) LDW_HIP(e.ensure(quiet));
    if (int rc = c->pin_lrc.reserve(64, "ensure_streams")) return rc;
    {   // the block-wide kernels (GEMM, screens) fill the chip; the tail of the previous block on the main stream is a chain of
        // small latency-bound kernels that should be dispatched as soon as they are ready: lowest priority for this stream
        int lo_p = 0, hi_p = 0;
        LDW_HIP(hipDeviceGetStreamPriorityRange(&lo_p, &hi_p));
        LDW_HIP(c->gemm_stream.ensure(hipStreamNonBlocking, lo_p));
    }
    // r05: what the streaming lr_links.tsv writer needs on the device side (ldw_lr_stream_begin): made here, not inside a job
    LDW_HIP(c->lr_st.ensure(hipStreamNonBlocking));
    for (auto &e : c->lr_ev) LDW_HIP(e.ensure(quiet));
    if (int rc = c->lr_counts.reserve(sizeof(int64_t) * 64, "ensure_streams")) return rc;
    if (int rc = c->lr_pin.reserve((size_t)32 << 20, "ensure_streams")) return rc;   // (2 M rows: a batch of eight items of a C4 pass is 0.2-0.6 M)
    c->streams_ready = true;
    return LDW_OK;
}

int join_prepare(ldw_ctx *c) {
    if (!c) return LDW_OK;
    int rc = LDW_OK;
    for (int which = 0; which < 2; ++which) {
        std::thread &t = which == 0 ? c->prep_thread : c->prep_thread2;
        if (t.joinable()) t.join();
        int &trc = which == 0 ? c->prep_rc : c->prep_rc2;
        if (trc != LDW_OK && rc == LDW_OK) {
            rc = trc;
            set_error("side thread of %s: %s", which == 0 ? "ldw_ctx_create" : "ldw_ctx_reserve", (which == 0 ? c->prep_err : c->prep_err2).c_str());
        }
        trc = LDW_OK;
    }
    return rc;
}

// ldw_ctx_reserve's side thread: the per-slot device buffers of a pass of blocks of `blk` SNPs (spans of up to nseg of them), from the estimated
// geometry of its largest item (slot_geom_estimate, ldw_slots.h) — whatever turns out too small grows where it is used, as before.
int reserve_slot_buffers(ldw_ctx *c, int64_t Npad, int64_t blk, int64_t nseg) {
    const int64_t KW = Npad / 64;
    const SlotGeom g = slot_geom_estimate(blk, nseg);
    const size_t RF = (size_t)g.RFpad, RT = (size_t)g.RTpad;
    const size_t cap = pair_cap_for(g.nf, g.nt, g.nseg);
    const size_t one = (size_t)blk * (size_t)blk;
    for (int s = 0; s < LDW_NSLOT; ++s) {
        if (int rc = c->panel[s][0].reserve(RF * (size_t)KW * 16)) return rc;   // (the scaled panel of k_pack_panel: 16 bytes per word)
        if (int rc = c->panel[s][1].reserve(RT * (size_t)KW * 16)) return rc;
        if (int rc = c->Gapx[s].reserve(RF * RT * 4)) return rc;
        if (int rc = UnitsLayout(g).reserve(c->apx_units[s])) return rc;
        if (int rc = PacksLayout(g).reserve(c->apx_packs[s])) return rc;
        if (int rc = MiniLayout(g).reserve(c->apx_mini[s])) return rc;
        if (int rc = PairsLayout((uint32_t)cap, maybe_cap_for(g.RTpad, g.RFpad)).reserve(c->pairs[s])) return rc;
        if (int rc = BinsLayout(g).reserve(c->apx_bins[s])) return rc;
        if (int rc = c->apx_clean[s].reserve((RT / 32) * (RF / 64) + 64)) return rc;
        if (int rc = c->hist[s].reserve((size_t)nseg * NBINS * 8)) return rc;
        const size_t cand = std::max<size_t>(one, (size_t)nseg * std::min<size_t>(one, (size_t)PAIR_PATHS * PAIR_SHARDS * cap));
        if (int rc = c->cand_key[s].reserve(cand * 8)) return rc;
        if (int rc = c->cand_val[s].reserve(cand * 8)) return rc;
        if (int rc = gx(c, s).reserve(RF * RF * 8)) return rc;   // the exact 5-limb sums of a single block's band tiles
    }
    if (int rc = c->pair_sums.reserve((size_t)PAIR_PATHS * PAIR_SHARDS * cap * 16 * 8)) return rc;
    return LDW_OK;
}

int block_mi_dense(ldw_ctx *c, const int32_t *from_idx, int64_t nf, const int32_t *to_idx, int64_t nt, int quirk) {
    EmitArgs E;
    memset(&E, 0, sizeof(E));
    return run_block_mi(c, from_idx, nf, to_idx, nt, quirk, E);
}

void warm_mi() {
    hipFuncAttributes a;
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_zero4));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void *>(&k_mi_screen<1, true>));
    (void)hipGetLastError();
}
}  // namespace ldw

extern "C" {

int ldw_mi_block(ldw_ctx *c, const int32_t *from_idx, int64_t nf, const int32_t *to_idx, int64_t nt, int quirk_mode,
                 double *MI_out, int on_device) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(from_idx && to_idx && MI_out, LDW_ERR_ARG, "ldw_mi_block: null argument");
    LDW_REQUIRE(quirk_mode == LDW_QUIRK_REFERENCE || quirk_mode == LDW_QUIRK_INTENDED, LDW_ERR_ARG, "bad quirk mode");
    EmitArgs E;
    memset(&E, 0, sizeof(E));
    if (int rc = run_block_mi(c, from_idx, nf, to_idx, nt, quirk_mode, E)) return rc;
    LDW_HIP(hipMemcpyAsync(MI_out, c->MIblk.p, (size_t)nf * nt * 8, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                           c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    float t01 = 0, t12 = 0;
    LDW_HIP(hipEventElapsedTime(&t01, c->ev[0], c->ev[1]));
    LDW_HIP(hipEventElapsedTime(&t12, c->ev[1], c->ev[2]));
    c->last_ms[0] = t01;
    c->last_ms[1] = t12;
    c->last_ms[2] = 0;
    c->last_ms[3] = t01 + t12;
    return LDW_OK;
}

int ldw_joint_tables(ldw_ctx *c, const int32_t *pair_a, const int32_t *pair_b, int64_t np, int64_t *counts_out,
                     int64_t *fixed_out, int *frac_bits_out) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(pair_a && pair_b && np > 0, LDW_ERR_ARG, "ldw_joint_tables: bad argument");
    if (int rc = join_prepare(c)) return rc;   // (ldw_ctx_reserve's side thread sizes c->G's neighbours gx(c, s) — no entry point touches them beside it)
    if (int rc = ensure_rows(c)) return rc;
    if (frac_bits_out) *frac_bits_out = c->wts.frac_bits;
    const int64_t CH = 1024;
    std::vector<int8_t> ones((size_t)c->Npad, 1);
    ldw::DevBuf d_ones, d_out, d_cmarg;
    int rc = LDW_OK;
    if ((rc = d_ones.reserve((size_t)c->Npad)) || (rc = d_out.reserve((size_t)CH * 25 * 8)) || (rc = d_cmarg.reserve((size_t)c->L * 40))) return rc;
    hipError_t he = hipMemcpyAsync(d_ones.p, ones.data(), ones.size(), hipMemcpyHostToDevice, c->stream);
    if (he != hipSuccess) return ldw::hip_fail(he, "memcpy ones", __FILE__, __LINE__);
    hipLaunchKernelGGL(k_slot_counts, dim3((unsigned)((c->L + 255) / 256)), dim3(256), 0, c->stream,
                       c->rows.counts.as<int32_t>(), c->rows.slot_meta.as<uint32_t>(), c->L, d_cmarg.as<int64_t>());
    for (int64_t p0 = 0; p0 < np && rc == LDW_OK; p0 += CH) {
        const int64_t n = std::min(CH, np - p0);
        SideLists SF, ST;
        if ((rc = build_side(c, pair_a + p0, n, SF))) break;
        if ((rc = build_side(c, pair_b + p0, n, ST))) break;
        const int RFpad = SF.Rpad, RTpad = ST.Rpad;
        if ((rc = upload_i32(c, c->rowlist_f, SF.rowlist)) || (rc = upload_i32(c, c->rowlist_t, ST.rowlist)) ||
            (rc = upload_i32(c, c->lrow_f, SF.lrow)) || (rc = upload_i32(c, c->lrow_t, ST.lrow)))
            break;
        std::vector<int32_t> vf(pair_a + p0, pair_a + p0 + n), vt(pair_b + p0, pair_b + p0 + n);
        if ((rc = upload_i32(c, c->idx_f, vf)) || (rc = upload_i32(c, c->idx_t, vt))) break;
        if (hipStreamSynchronize(c->stream) != hipSuccess) { rc = LDW_ERR_HIP; break; }
        if ((rc = c->G.reserve((size_t)RFpad * RTpad * 8))) break;
        for (int pass = 0; pass < 2 && rc == LDW_OK; ++pass) {
            int64_t *host_out = pass == 0 ? counts_out : fixed_out;
            if (!host_out) continue;
            rc = launch_gemm_bits(c, c->rows.Mbits.as<uint64_t>(), c->KW, c->rowlist_t.as<int32_t>(), RTpad, c->rowlist_f.as<int32_t>(), RFpad, c->G.as<int64_t>(),
                                  pass == 0 ? 1 : c->wts.nlimbs, pass == 0 ? d_ones.as<int8_t>() : c->wts.digits.as<int8_t>(), 0);
            if (rc) break;
            hipLaunchKernelGGL(k_tables, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, c->G.as<int64_t>(), RFpad,
                               c->idx_f.as<int32_t>(), c->lrow_f.as<int32_t>(), c->idx_t.as<int32_t>(),
                               c->lrow_t.as<int32_t>(), (int)n, c->rows.slot_meta.as<uint32_t>(),
                               pass == 0 ? d_cmarg.as<int64_t>() : c->rows.slot_pfix.as<int64_t>(), d_out.as<int64_t>());
            he = hipMemcpyAsync(host_out + p0 * 25, d_out.p, (size_t)n * 25 * 8, hipMemcpyDeviceToHost, c->stream);
            if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
            if (he != hipSuccess) rc = ldw::hip_fail(he, "joint tables copy", __FILE__, __LINE__);
        }
    }
    return rc;
}

int ldw_links_begin(ldw_ctx *c, int64_t nblocks_capacity) {
    if (int rc = check_gpu(c)) return rc;
    if (int rc = join_prepare(c)) return rc;
    LDW_REQUIRE(nblocks_capacity > 0, LDW_ERR_ARG, "ldw_links_begin: capacity must be positive");
    if (c->links.blk_capacity != 0) {
        // the previous pass never reached ldw_links_end (an error return in the middle of ldw_mi_all_pairs / ldw_mi_block_links): kernels of
        // the aborted pass may still be queued on the three streams and read the index lists, staging images and per-slot buffers
        // that this pass is about to overwrite
        if (c->gemm_stream) LDW_HIP(hipStreamSynchronize(c->gemm_stream));
        if (c->copy_stream) LDW_HIP(hipStreamSynchronize(c->copy_stream));
        LDW_HIP(hipStreamSynchronize(c->stream));
        c->links.blk_capacity = 0;
    }
    if (int rc = ensure_rows(c)) return rc;  // uses ctx->small for staging; link bookkeeping takes it over below
    const size_t need = 64 + (size_t)LDW_NSLOT * LDW_SPAN_MAX * PICK_STRIDE + (size_t)nblocks_capacity * 32 + 64;
    if (int rc = c->small.reserve(need)) return rc;
    LDW_HIP(hipMemsetAsync(c->small.p, 0, need, c->stream));
    if (int rc = ensure_streams(c)) return rc;
    // everything queued on the main stream so far (row map, weights) must be visible to the GEMM stream
    LDW_HIP(hipEventRecord(c->ev_up[0], c->stream));
    LDW_HIP(hipStreamWaitEvent(c->gemm_stream, c->ev_up[0], 0));
    while ((int64_t)c->ev_pool.size() < nblocks_capacity * EVB) {
        ldw::Event e;
        LDW_HIP(e.ensure());
        c->ev_pool.push_back(std::move(e));
    }
    for (int k = 0; k < LDW_NSLOT; ++k) c->done_recorded[k] = false;
    c->early_sr = false;
    c->ev_valid.assign((size_t)nblocks_capacity, 1);
    c->lrc_recorded = false;
    c->links.new_pass();
    c->trace.clear();
    c->links.blk_capacity = nblocks_capacity;
    c->links.blk_cursor = 0;
    for (int i = 0; i < 4; ++i) c->last_ms[i] = 0;
    return LDW_OK;
}

static int links_check(ldw_ctx *c, const ldw_mi_params *p) {
    LDW_REQUIRE(c->links.blk_capacity > 0 && c->links.blk_cursor < c->links.blk_capacity, LDW_ERR_STATE,
                "call ldw_links_begin with enough capacity first");
    LDW_REQUIRE(p->sr_only || p->lr_links_approx > 0, LDW_ERR_ARG, "lr_links_approx must be positive");
    LDW_REQUIRE(p->quirk_mode == LDW_QUIRK_REFERENCE || p->quirk_mode == LDW_QUIRK_INTENDED, LDW_ERR_ARG, "bad quirk mode");
    LDW_REQUIRE(c->meta.have_meta, LDW_ERR_STATE, "SNP meta data (POS, g) not set");
    return LDW_OK;
}

int ldw_mi_block_links(ldw_ctx *c, const int32_t *from_idx, int64_t nf, const int32_t *to_idx, int64_t nt,
                       const ldw_mi_params *p) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(from_idx && to_idx && p, LDW_ERR_ARG, "ldw_mi_block_links: null argument");
    if (int rc = links_check(c, p)) return rc;
    SmallLayout sl;
    links_layout(c, sl);
    HostBlock hb;
    if (int rc = prep_block(c, from_idx, nf, to_idx, nt, p, (int)(c->links.blk_cursor % LDW_NSLOT), c->links.blk_cursor, hb)) return rc;
    if (int rc = submit_a(c, hb, p, sl)) return rc;
    if (int rc = submit_b(c, hb, p, sl)) return rc;
    if (int rc = finish_block(c, hb, p, sl)) return rc;
    ++c->links.blk_cursor;
    return LDW_OK;
}

int ldw_links_end(ldw_ctx *c) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(c->links.blk_capacity > 0, LDW_ERR_STATE, "ldw_links_end without ldw_links_begin");
    SmallLayout sl;
    links_layout(c, sl);
    const int64_t nb = c->links.blk_cursor;
    int64_t h_lr = 0;
    std::vector<int64_t> si((size_t)nb * 3 + 1);
    std::vector<double> sd((size_t)nb + 1);
    int64_t h_viol = 0, h_apx[3] = {0, 0, 0};
    LDW_HIP(hipMemcpyAsync(&h_lr, sl.lr_count, 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemcpyAsync(&h_viol, sl.lr_count + 1, 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipMemcpyAsync(h_apx, sl.lr_count + 2, 24, hipMemcpyDeviceToHost, c->stream));
    unsigned long long h_skip = 0;
    if (c->apx_skip.p) {   // wave tiles the approximate GEMMs pruned: not executed work (ldw_gemm_stats)
        LDW_HIP(hipMemcpyAsync(&h_skip, c->apx_skip.p, 8, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipMemsetAsync(c->apx_skip.p, 0, 8, c->stream));
    }
    if (nb > 0) {
        LDW_HIP(hipMemcpyAsync(si.data(), sl.stats_i, (size_t)nb * 24, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipMemcpyAsync(sd.data(), sl.stats_d, (size_t)nb * 8, hipMemcpyDeviceToHost, c->stream));
    }
    LDW_HIP(hipStreamSynchronize(c->stream));
    c->links.n_lr = h_lr;
    c->cnt.screen_violations += h_viol;
    c->cnt.apx_units_listed += h_apx[0];
    c->cnt.apx_pairs_listed += h_apx[1];
    c->cnt.maybe_entries += h_apx[2];
    c->cnt.apx_waves_skipped += (int64_t)h_skip;
    c->cnt.gemm_stat[1] -= (double)h_skip * c->apx_ops_per_wave;
    c->links.stats.resize((size_t)nb);
    for (int64_t b = 0; b < nb; ++b) {
        c->links.stats[b].n_lr_total = si[b * 3 + 0];
        c->links.stats[b].n_lr_kept = si[b * 3 + 1];
        c->links.stats[b].n_sr = si[b * 3 + 2];
        c->links.stats[b].disc_thresh = sd[b];
        float t01 = 0, t12 = 0, t23 = 0;
        const hipEvent_t *ev = handles(&c->ev_pool[(size_t)b * EVB]);
        if (b < (int64_t)c->ev_valid.size() && !c->ev_valid[(size_t)b]) continue;   // a later segment of a span: its time is in the span's first block
        LDW_HIP(hipEventElapsedTime(&t01, ev[0], ev[1]));
        LDW_HIP(hipEventElapsedTime(&t12, ev[c->knobs.engine == LDW_ENGINE_MFMA ? 4 : 1], ev[2]));
        if (c->knobs.engine == LDW_ENGINE_MFMA) {   // the screens of the approximate path run behind the GEMM on its stream
            float t15 = 0;
            if (hipEventElapsedTime(&t15, ev[1], ev[5]) == hipSuccess) t12 += t15;
            else (void)hipGetLastError();   // (an event this block never recorded: the failed query must not surface at the next launch check)
        }
        LDW_HIP(hipEventElapsedTime(&t23, ev[2], ev[3]));
        c->last_ms[0] += t01;
        c->last_ms[1] += t12;
        c->last_ms[2] += t23;
        c->last_ms[3] += t01 + t12 + t23;
        static const bool trace_on = getenv("LDW_BLOCK_TRACE") != nullptr;
        if (trace_on && b < (int64_t)c->trace.size()) {
            const ldw::BlockTrace &tr = c->trace[(size_t)b];
            float span = 0;
            int64_t pb = b - 1;
            while (pb >= 0 && pb < (int64_t)c->ev_valid.size() && !c->ev_valid[(size_t)pb]) --pb;   // (the previous block that recorded events: a span's first)
            if (pb >= 0 && hipEventElapsedTime(&span, c->ev_pool[(size_t)pb * EVB + 3], ev[3]) != hipSuccess) (void)hipGetLastError();   // selection end of the item before -> selection end of b
            fprintf(stderr, "[ldw block %3lld] %s path %d guess %4d true %4d%s cand %8lld kept %7lld  gemm %.3f epi %.3f sel %.3f  span %.3f ms\n", (long long)b,
                    tr.diag ? "diag" : "off ", tr.path, tr.guess, tr.B_true, tr.missed ? " MISS" : "", tr.n_cand, (long long)c->links.stats[b].n_lr_kept, t01, t12, t23, span);
        }
    }
    c->links.blk_capacity = 0;
    return LDW_OK;
}

// A pass over a block list: the plan, the helpers, the table sizing, the probes and the item loop are ldw_mi_pass.inc's (and ldw_pass_plan.h's).
int ldw_mi_all_pairs(ldw_ctx *c, const int32_t *blocks, int64_t nblocks, const ldw_mi_params *p, int reset) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(blocks && p && nblocks > 0, LDW_ERR_ARG, "ldw_mi_all_pairs: bad argument");
    LDW_REQUIRE(reset, LDW_ERR_ARG, "ldw_mi_all_pairs: appending to earlier calls is not supported (reset must be 1)");
    const bool host_timing = ldw::host_timing();
    using Clock = HostClock;
    const Clock::Point t_enter = Clock::now();
    if (int rc = join_prepare(c)) return rc;
    const Clock::Point t_joined = Clock::now();
    if (int rc = ldw_links_begin(c, nblocks)) return rc;
    if (int rc = links_check(c, p)) return rc;
    const Clock::Point t_begun = Clock::now();
    SmallLayout sl;
    links_layout(c, sl);
    const PassPlan plan = plan_pass(c, blocks, nblocks, p);
    ItemLoop loop(c, blocks, p, sl, plan.items);   // (every return below joins the helpers: ~ItemLoop)
    c->early_sr = plan.spans;                      // read by the helpers: stored before the first one starts
    loop.start_helpers();
    if (int rc = size_link_tables(c, blocks, nblocks, p)) return rc;
    const Clock::Point t_sized = Clock::now();
    Probes probes;
    if (plan.probes_wanted)
        if (int rc = queue_probes(c, blocks, nblocks, p, sl, probes)) return rc;
    const Clock::Point t_queued = Clock::now();
    // The first item's lists go up while the probes run (the upload needs no guess); then the host waits for the probes that item needs.
    if (int rc = loop.wait_prepared(0)) return rc;
    if (int rc = submit_upload(c, loop.hb[0])) return rc;
    if (int rc = collect_probes_for(c, loop.hb[0], probes)) return rc;
    const Clock::Point t_probed = Clock::now();
    if (int rc = loop.submit_next()) return rc;
    const Clock::Point t_planned = Clock::now();
    if (host_timing)
        fprintf(stderr, "[ldw host us] waiting for the side threads %.0f  links_begin (row map if stale, bookkeeping) %.0f  table sizing + plan + helper start %.0f  cold-start probes queued %.0f  first upload + wait for its probe %.0f  first item submitted %.0f\n",
                Clock::us(t_enter, t_joined), Clock::us(t_joined, t_begun), Clock::us(t_begun, t_sized), Clock::us(t_sized, t_queued), Clock::us(t_queued, t_probed), Clock::us(t_probed, t_planned));
    if (loop.run(probes) != LDW_OK) return loop.drain_after_failure();
    const Clock::Point t_loop = Clock::now();
    const int rc_end = ldw_links_end(c);
    if (host_timing) {
        const double n = (double)loop.nitems;
        fprintf(stderr, "[ldw host us] item loop %.0f  links_end %.0f  whole call %.0f\n", Clock::us(t_planned, t_loop), Clock::us(t_loop, Clock::now()), Clock::us(t_enter, Clock::now()));
        fprintf(stderr, "[ldw host us/item] submit_b %.1f  wait for the helper's prep %.1f  submit_a (incl. that wait) %.1f  finish (incl. wait) %.1f  items %lld (blocks %lld)\n", loop.th[0] / n, loop.th[1] / n,
                loop.th[2] / n, loop.th[3] / n, (long long)loop.nitems, (long long)nblocks);
    }
    return rc_end;
}

int ldw_sr_pairs_fill(ldw_ctx *c, const int32_t *blocks, int64_t nblocks, double sr_dist, int32_t *a_out, int32_t *b_out, int64_t capacity, int64_t *n_out) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(blocks && nblocks > 0 && n_out && sr_dist >= 0, LDW_ERR_ARG, "ldw_sr_pairs_fill: bad argument");
    LDW_REQUIRE(c->meta.have_meta && c->meta.pos_sorted, LDW_ERR_STATE, "ldw_sr_pairs_fill: needs SNP positions in ascending order (ldw_set_snp_meta)");
    *n_out = 0;
    // r05: everything on the device (k_cols_dev ... k_sr_fill_all) — the host loop below built the intervals of C4's 20 band blocks in 17 ms, which a
    // multi-GPU job's rank 0 paid after every gather.  Integral genome length (every len is then an exact integer on host and device alike); a column
    // whose interval check fails (none on ascending positions) sends the call down the host path, as does LDW_SR_PAIRS_HOST=1 (A/B, tests).
    // A block whose positions do not lie within one turn of the circle (within_one_turn, ldw_pass_plan.h) raises `bad` before anything is launched: the
    // windows of k_cols_dev are not exact there and its boundary checks do not see it; build_cols scans such a block with the predicate.
    const std::vector<int32_t> &Ph = c->meta.h_POS;
    auto block_in_one_turn = [&](int32_t fs, int32_t fe, int32_t ts, int32_t te) {   // (POS ascends: a side's ends are its extremes)
        return within_one_turn((double)std::min(Ph[(size_t)fs - 1], Ph[(size_t)ts - 1]), (double)std::max(Ph[(size_t)fe - 1], Ph[(size_t)te - 1]), c->meta.g);
    };
    bool bad_turn = false;
    for (int64_t b = 0; b < nblocks && !bad_turn; ++b) {
        if (int rc = check_block(c, blocks, b)) return rc;
        bad_turn = !block_in_one_turn(blocks[b * 4 + 0], blocks[b * 4 + 1], blocks[b * 4 + 2], blocks[b * 4 + 3]);
    }
    if (!bad_turn && c->meta.g == std::floor(c->meta.g) && getenv("LDW_SR_PAIRS_HOST") == nullptr) {
        std::vector<SrBlkDev> hb;
        int64_t ncols = 0;
        for (int64_t b = 0; b < nblocks; ++b) {
            const int32_t fs = blocks[b * 4 + 0], fe = blocks[b * 4 + 1], ts = blocks[b * 4 + 2], te = blocks[b * 4 + 3];
            if (int rc = check_block(c, blocks, b)) return rc;
            if (ts > fe && 2 * sr_dist < c->meta.g) {   // (as below: ranges further apart than sr_dist directly and across the origin)
                const double pf_min = Ph[(size_t)fs - 1], pf_max = Ph[(size_t)fe - 1], pt_min = Ph[(size_t)ts - 1], pt_max = Ph[(size_t)te - 1];
                if (pt_min - pf_max > sr_dist && pf_min + c->meta.g - pt_max > sr_dist) continue;
            }
            hb.push_back(SrBlkDev{fs - 1, fe - fs + 1, ts - 1, te - ts + 1, (fs == ts && fe == te) ? 1 : 0, 0, ncols});
            ncols += te - ts + 1;
        }
        if (hb.empty()) return LDW_OK;
        const size_t nb = hb.size();
        Carve cv;   // the blocks, their columns' upper / lower counts, the blocks' rows and first rows, the flag of a column that needs the host
        auto d_blk = cv.take<SrBlkDev>((int64_t)nb);
        auto d_cu = cv.take<int32_t>(ncols), d_cl = cv.take<int32_t>(ncols);
        auto d_rows = cv.take<int64_t>((int64_t)nb), d_base = cv.take<int64_t>((int64_t)nb + 1);
        auto d_bad = cv.take<int>(2);
        if (int rc = cv.reserve(c->srm.seg)) return rc;
        if (int rc = c->srm.out.reserve((size_t)ncols * sizeof(ColInfo))) return rc;
        ColInfo *d_cols = c->srm.out.as<ColInfo>();
        LDW_HIP(hipMemcpyAsync(d_blk, hb.data(), nb * sizeof(SrBlkDev), hipMemcpyHostToDevice, c->stream));
        LDW_HIP(hipMemsetAsync(d_bad, 0, 8, c->stream));
        hipLaunchKernelGGL(k_cols_dev, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, c->stream, c->meta.POS.as<int32_t>(), c->meta.g, sr_dist, d_blk, (int)nb, ncols, d_cols, d_cu,
                           d_cl, d_bad);
        hipLaunchKernelGGL(k_cols_scan, dim3((unsigned)nb), dim3(256), 0, c->stream, d_blk, d_cols, d_cu, d_cl, d_rows);
        hipLaunchKernelGGL(k_blk_bases, dim3(1), dim3(64), 0, c->stream, d_rows, (int)nb, d_base);
        LDW_HIP(hipGetLastError());
        int64_t total = 0;
        int bad = 0;
        LDW_HIP(hipMemcpyAsync(&total, d_base + nb, 8, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipStreamSynchronize(c->stream));
        if (!bad) {
            *n_out = total;
            if (total > 0 && a_out && b_out) {
                LDW_REQUIRE(total <= capacity, LDW_ERR_SIZE, "ldw_sr_pairs_fill: capacity %lld < %lld rows", (long long)capacity, (long long)total);
                hipLaunchKernelGGL(k_sr_fill_all, dim3((unsigned)((ncols + 3) / 4)), dim3(256), 0, c->stream, d_cols, d_blk, (int)nb, ncols, d_base, a_out, b_out);
                LDW_HIP(hipGetLastError());
                LDW_HIP(hipStreamSynchronize(c->stream));
            }
            return LDW_OK;
        }
    }
    std::vector<int32_t> fi, ti;
    std::vector<ColInfo> cols2[2];
    int64_t base = 0;
    // r05: two record buffers in turn (the upload of block b + 1 no longer waits for the kernel of block b: one stream synchronisation per block
    // made this 12 ms for C4's 55 blocks), and the block pairs whose ranges lie further apart than sr_dist on the circle — 35 of the 55 — are
    // recognised from their four end positions (POS ascends) without building their columns.
    ldw::DevBuf dcols[2];
    ldw::Event done[2];
    const std::vector<int32_t> &P = c->meta.h_POS;
    int64_t n_filled = 0;
    for (int64_t b = 0; b < nblocks; ++b) {
        const int32_t fs = blocks[b * 4 + 0], fe = blocks[b * 4 + 1], ts = blocks[b * 4 + 2], te = blocks[b * 4 + 3];
        if (int rc = check_block(c, blocks, b)) return rc;
        if (ts > fe && 2 * sr_dist < c->meta.g && block_in_one_turn(fs, fe, ts, te)) {   // disjoint ranges, to side after the from side: no pair within sr_dist directly or across the origin?
            const double pf_min = P[(size_t)fs - 1], pf_max = P[(size_t)fe - 1], pt_min = P[(size_t)ts - 1], pt_max = P[(size_t)te - 1];
            if (pt_min - pf_max > sr_dist && pf_min + c->meta.g - pt_max > sr_dist) continue;
        }
        const int64_t nf = fe - fs + 1, nt = te - ts + 1;
        fi.resize((size_t)nf);
        ti.resize((size_t)nt);
        for (int64_t k = 0; k < nf; ++k) fi[(size_t)k] = fs - 1 + (int32_t)k;
        for (int64_t k = 0; k < nt; ++k) ti[(size_t)k] = ts - 1 + (int32_t)k;
        const bool diag = fs == ts && fe == te;
        int64_t n_blk = 0;
        const int k = (int)(n_filled & 1);
        if (done[k]) LDW_HIP(hipEventSynchronize(done[k]));   // (the upload and the kernel that used this pair of buffers two blocks ago)
        std::vector<ColInfo> &cols = cols2[k];
        if (int rc = build_cols(c, fi.data(), nf, ti.data(), nt, diag, sr_dist, cols, n_blk)) return rc;
        if (n_blk > 0 && a_out && b_out) {
            LDW_REQUIRE(base + n_blk <= capacity, LDW_ERR_SIZE, "ldw_sr_pairs_fill: capacity %lld < %lld rows", (long long)capacity, (long long)(base + n_blk));
            LDW_HIP(done[k].ensure(hipEventDisableTiming));
            if (int rc = dcols[k].reserve(cols.size() * sizeof(ColInfo))) return rc;
            LDW_HIP(hipMemcpyAsync(dcols[k].p, cols.data(), cols.size() * sizeof(ColInfo), hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(k_sr_fill, dim3((unsigned)((nt + 3) / 4)), dim3(256), 0, c->stream, dcols[k].as<ColInfo>(), (int)nf, (int)nt, fs - 1, ts - 1, diag ? 1 : 0, base,
                               a_out, b_out);
            LDW_HIP(hipGetLastError());
            LDW_HIP(hipEventRecord(done[k], c->stream));
            ++n_filled;
        }
        base += n_blk;
    }
    LDW_HIP(hipStreamSynchronize(c->stream));
    *n_out = base;
    return LDW_OK;
}

// inspection only: the first 16 pairs verify mode counted as violations since the library was loaded — (from SNP, to SNP, exact MI, the level they were judged against) —
// and how many there were; resets the record.  out: 1 + 64 doubles.
int ldw_debug_violations(ldw_ctx *c, double *out) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(out, LDW_ERR_ARG, "ldw_debug_violations: null output");
    LDW_HIP(hipDeviceSynchronize());
    unsigned long long n = 0, zero = 0;
    LDW_HIP(hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_viol_n), 8));
    LDW_HIP(hipMemcpyFromSymbol(out + 1, HIP_SYMBOL(g_viol_rec), 64 * 8));
    LDW_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_viol_n), &zero, 8));
    out[0] = (double)n;
    return LDW_OK;
}

int ldw_debug_tab11(ldw_ctx *c, double W, double lo, double delta, double eta, double sprime, int32_t *out, double *cbin_out) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(out && cbin_out && W > 0 && lo > 0 && delta >= 0 && eta >= 0 && sprime > 0, LDW_ERR_ARG, "ldw_debug_tab11: bad argument");
    constexpr int NB = 64;
    ldw::DevBuf t;
    if (int rc = t.reserve((size_t)NB * NB * 8)) return rc;
    const float cbin = (float)(NB / std::sqrt(W + 1.0));
    hipLaunchKernelGGL(ldw::k_build_tab11, dim3(NB * NB * 32 / 256), dim3(256), 0, c->stream, W, lo, delta, eta, sprime, NB, cbin, t.as<int2>());
    hipError_t he = hipGetLastError();
    if (he == hipSuccess) he = hipMemcpyAsync(out, t.p, (size_t)NB * NB * 8, hipMemcpyDeviceToHost, c->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
    if (he != hipSuccess) return ldw::hip_fail(he, "ldw_debug_tab11", __FILE__, __LINE__);
    *cbin_out = (double)cbin;
    return LDW_OK;
}

int ldw_slot_report(ldw_ctx *c, int64_t out[6]) {
    LDW_REQUIRE(c && out, LDW_ERR_ARG, "ldw_slot_report: null argument");
    if (int rc = join_prepare(c)) return rc;   // (ldw_ctx_reserve's side thread may still be sizing the buffers)
    for (int k = 1; k < 6; ++k) out[k] = 0;
    out[0] = c->cnt.slot_grown;
    for (int s = 0; s < LDW_NSLOT; ++s) {
        out[1] += (int64_t)c->apx_units[s].cap;
        out[2] += (int64_t)c->apx_packs[s].cap;
        out[3] += (int64_t)c->pairs[s].cap;
        out[4] += (int64_t)c->apx_bins[s].cap;
        out[5] += (int64_t)c->apx_mini[s].cap;
    }
    return LDW_OK;
}

int ldw_set_pair_cap(uint32_t cap) {
    LDW_REQUIRE(cap == 0 || (cap >= 16 && cap <= (1u << 22)), LDW_ERR_ARG, "ldw_set_pair_cap: 0 or 16..2^22");
    g_pair_cap_override.store(cap);
    return LDW_OK;
}

int ldw_links_count(ldw_ctx *c, int which, int64_t *n_out) {
    LDW_REQUIRE(c && n_out && (which == 0 || which == 1), LDW_ERR_ARG, "ldw_links_count: bad argument");
    *n_out = which == 0 ? c->links.n_sr : c->links.n_lr;
    return LDW_OK;
}

int ldw_links_device_ptrs(ldw_ctx *c, int which, const int32_t **a_out, const int32_t **b_out, const double **MI_out, int64_t *n_out) {
    if (int rc = check_gpu(c)) return rc;
    if (int rc = join_prepare(c)) return rc;
    LDW_REQUIRE((which == 0 || which == 1) && a_out && b_out && MI_out && n_out, LDW_ERR_ARG, "ldw_links_device_ptrs: bad argument");
    LDW_REQUIRE(c->links.blk_capacity == 0, LDW_ERR_STATE, "ldw_links_device_ptrs: a link pass is still open (ldw_links_end)");
    LDW_HIP(hipStreamSynchronize(c->stream));
    *a_out = (which == 0 ? c->links.sr_a : c->links.lr_a).as<int32_t>();
    *b_out = (which == 0 ? c->links.sr_b : c->links.lr_b).as<int32_t>();
    *MI_out = (which == 0 ? c->links.sr_mi : c->links.lr_mi).as<double>();
    *n_out = which == 0 ? c->links.n_sr : c->links.n_lr;
    return LDW_OK;
}

#ifdef LDW_SCREEN_STATS
int ldw_debug_screen_stats(unsigned long long *out16) {   // (measurement build only; not in the header)
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(ldw::g_scr_stats), 16 * 8) != hipSuccess) return LDW_ERR_HIP;
    return LDW_OK;
}
#endif
int ldw_links_fetch(ldw_ctx *c, int which, int32_t *a_out, int32_t *b_out, double *MI_out, int64_t capacity,
                    int on_device) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(which == 0 || which == 1, LDW_ERR_ARG, "ldw_links_fetch: which must be 0 (sr) or 1 (lr)");
    const int64_t n = which == 0 ? c->links.n_sr : c->links.n_lr;
    LDW_REQUIRE(capacity >= n, LDW_ERR_SIZE, "ldw_links_fetch: capacity %lld < %lld rows", (long long)capacity, (long long)n);
    if (n == 0) return LDW_OK;
    LDW_REQUIRE(a_out && b_out && MI_out, LDW_ERR_ARG, "ldw_links_fetch: null output");
    const hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    ldw::DevBuf &A = which == 0 ? c->links.sr_a : c->links.lr_a, &B = which == 0 ? c->links.sr_b : c->links.lr_b, &M = which == 0 ? c->links.sr_mi : c->links.lr_mi;
    LDW_HIP(hipMemcpyAsync(a_out, A.p, (size_t)n * 4, k, c->stream));
    LDW_HIP(hipMemcpyAsync(b_out, B.p, (size_t)n * 4, k, c->stream));
    LDW_HIP(hipMemcpyAsync(MI_out, M.p, (size_t)n * 8, k, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    return LDW_OK;
}

int ldw_links_import(ldw_ctx *c, int which, const int32_t *a, const int32_t *b, const double *MI, int64_t n, int on_device) {
    if (int rc = check_gpu(c)) return rc;
    if (int rc = join_prepare(c)) return rc;
    LDW_REQUIRE(which == 0 || which == 1, LDW_ERR_ARG, "ldw_links_import: which must be 0 (sr) or 1 (lr)");
    LDW_REQUIRE(n >= 0 && (n == 0 || (a && b && MI)), LDW_ERR_ARG, "ldw_links_import: bad argument");
    LDW_REQUIRE(c->links.blk_capacity == 0, LDW_ERR_STATE, "ldw_links_import: a link pass is still open (ldw_links_end)");
    if (c->gemm_stream) LDW_HIP(hipStreamSynchronize(c->gemm_stream));
    ldw::DevBuf &A = which == 0 ? c->links.sr_a : c->links.lr_a, &B = which == 0 ? c->links.sr_b : c->links.lr_b, &M = which == 0 ? c->links.sr_mi : c->links.lr_mi;
    if (int rc = A.reserve((size_t)std::max<int64_t>(n, 1) * 4)) return rc;
    if (int rc = B.reserve((size_t)std::max<int64_t>(n, 1) * 4)) return rc;
    if (int rc = M.reserve((size_t)std::max<int64_t>(n, 1) * 8)) return rc;
    if (n > 0) {
        const hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        LDW_HIP(hipMemcpyAsync(A.p, a, (size_t)n * 4, k, c->stream));
        LDW_HIP(hipMemcpyAsync(B.p, b, (size_t)n * 4, k, c->stream));
        LDW_HIP(hipMemcpyAsync(M.p, MI, (size_t)n * 8, k, c->stream));
        LDW_HIP(hipStreamSynchronize(c->stream));
    }
    (which == 0 ? c->links.n_sr : c->links.n_lr) = n;
    c->links.replaced(c->kept);
    return LDW_OK;
}

int ldw_block_stats(ldw_ctx *c, int64_t nblocks, int64_t *n_lr_total, int64_t *n_lr_kept, int64_t *n_sr,
                    double *disc_thresh) {
    LDW_REQUIRE(c, LDW_ERR_ARG, "null context");
    LDW_REQUIRE((int64_t)c->links.stats.size() == nblocks, LDW_ERR_ARG, "ldw_block_stats: last call processed %lld blocks, not %lld",
                (long long)c->links.stats.size(), (long long)nblocks);
    for (int64_t b = 0; b < nblocks; ++b) {
        if (n_lr_total) n_lr_total[b] = c->links.stats[b].n_lr_total;
        if (n_lr_kept) n_lr_kept[b] = c->links.stats[b].n_lr_kept;
        if (n_sr) n_sr[b] = c->links.stats[b].n_sr;
        if (disc_thresh) disc_thresh[b] = c->links.stats[b].disc_thresh;
    }
    return LDW_OK;
}

}  // extern "C"
