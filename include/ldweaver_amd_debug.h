/*
 * ldweaver_amd_debug.h — diagnostics, test hooks and execution options of libldweaver_amd.so.
 *
 * Nothing here is needed to integrate the engine: the integration surface is ldweaver_amd.h, which this
 * header includes.  What is declared here falls into four groups:
 *   - counters, timings and reports of what a context did (measurement, the benchmark's roofline);
 *   - execution options: which path, stream overlap or screen the all-pairs loop uses.  Every MI that is
 *     emitted is computed from the exact fixed-point sums on every path, so the link tables do not depend
 *     on any of them;
 *   - inspection entry points that return intermediate values the reference never materialises;
 *   - test hooks that expose the engine's bounds and kernels as functions (BOUNDS.md, tests/test_bounds.py).
 * The same conventions hold as in ldweaver_amd.h: int status, ldw_last_error(), caller-allocated outputs.
 * Past measurements behind these switches are recorded in DESIGN.md and docs/HISTORY.md.
 */
#ifndef LDWEAVER_AMD_DEBUG_H
#define LDWEAVER_AMD_DEBUG_H

#include "ldweaver_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LDW_ENGINE_MFMA 0 /* i8 MFMA fixed-point co-occurrence GEMM + fp64 epilogue (default) */
#define LDW_ENGINE_HIST 1 /* joint histograms on bit planes: LDS-tiled class-wise popcounts (VALU), exact int64 sums, same fp64 epilogue and results */
#define LDW_ENGINE_HIST_STATES 2 /* removed (byte-state histogram kernel, measured ~200x slower): ldw_set_engine answers LDW_ERR_STATE */

/* ---- library / context -------------------------------------------------------------------------------------------------------- */
/* build flags; always 0 (bit 0 once marked a build with the measured-slower variants, which have been removed) */
int ldw_build_info(void);
/* elapsed ms of the kernels of the last ldw_mi_block / ldw_mi_all_pairs call, by stage, measured with
 * HIP events on the context's stream: [0] gemm, [1] epilogue, [2] selection, [3] total */
int ldw_ctx_last_timing(ldw_ctx *ctx, double ms_out[4]);
/* diagnostics since the context was created: out[0] = blocks whose speculative long-range gather had to fall back to
 * the dense pass, out[1] = 0 (was: blocks run by the removed fused kernel), out[2] = blocks run by the two-kernel path,
 * out[3] = pairs the fp32 screen would have lost (counted in ldw_set_screen mode 2 only; must stay 0) */
int ldw_ctx_counters(ldw_ctx *ctx, int64_t out[4]);
/* the same four, then out[4] = blocks run in the mixed-precision path (ldw_set_mixed), out[5] = blocks run in the
 * approximate-GEMM path (ldw_set_path), out[6] = units its screen listed (they hold a short-range pair), out[7] = long-range candidate
 * pairs its screen listed */
int ldw_ctx_counters2(ldw_ctx *ctx, int64_t out[8]);
/* Work the block-wide GEMMs of this context EXECUTED since the last reset (for the roofline: executed int8 operations /
 * kernel time / peak): out[0] launches and out[1] int8 operations (2 x rows x rows x positions of the wave tiles that do not exit
 * at once) of the approximate GEMM (gemm_apx_kernel), out[2] / out[3] the same for the unmasked limb GEMM (gemm_bits_kernel<J>,
 * all J limbs), out[4] launches of the band-masked limb GEMM, out[5] launches of the approximate GEMM that applied the threshold
 * table in their epilogue (long-range-only blocks).  reset != 0 clears the counts. */
int ldw_gemm_stats(ldw_ctx *ctx, double out[6], int reset);
/* diagnostics of the approximate path after ldw_set_weights: out[0] = usable (0/1), out[1] = max relative error delta of the
 * dual-digit weights, out[2] = weight classes, out[3] = popcount segments, out[4] = exponent transitions, out[5] = e_last */
int ldw_apx_info(ldw_ctx *ctx, double out[6]);

/* ---- Hamming weights and joint tables --------------------------------------------------------------------------------------- */
/* What the last ldw_hamming_weights of this context did, for its roofline (bench.py `roofline_hamming`): out[0] = bit columns K (one per
 * minor state + one "not the major state" column per multi-allelic SNP: ~1.3 L), [1] = K padded to the GEMM's word pairs, [2] = ms of the
 * kernels in front of the GEMM (column bits, bit transpose, per-sequence counts; HIP events), [3] = ms of the lower-triangular int8 GEMM,
 * [4] = ms of the N x N neighbour count, [5] / [6] = algorithmic bytes of the kernels in front of / behind the GEMM, [7] = wall ms of the
 * whole call on the host (allocations, state counts, column list, uploads included).  The GEMM's executed int8 operations are in
 * ldw_gemm_stats (bits_ops). */
int ldw_hamming_stats(ldw_ctx *ctx, double out[8]);
/* inspection: exact weighted joint tables in fixed point and plain integer joint counts for a list of SNP pairs:
 * counts_out[p][25] (row X of SNP a, column Y of SNP b), fixed_out[p][25] (sum of quantised weights,
 * value = fixed * 2^-frac_bits).  Either output may be NULL. */
int ldw_joint_tables(ldw_ctx *ctx, const int32_t *pair_a, const int32_t *pair_b, int64_t npairs,
                     int64_t *counts_out, int64_t *fixed_out, int *frac_bits_out);

/* ---- execution options of the all-pairs loop: results do not depend on them ----------------------------------------------- */
/* LDW_ENGINE_MFMA (default) or LDW_ENGINE_HIST; LDW_ENGINE_HIST_STATES answers LDW_ERR_STATE */
int ldw_set_engine(ldw_ctx *ctx, int engine);
/* on (default): the co-occurrence GEMM of block b+1 runs on a second stream beside the epilogue and link selection
 * of block b (~5 % faster end to end).  off: all kernels of all blocks run back to back on the context's stream, so
 * that the per-stage times of ldw_ctx_last_timing are exclusive kernel times (what bench.py's roofline uses). */
int ldw_set_overlap(ldw_ctx *ctx, int on);
/* 0: GEMM -> G in HBM -> k_mi_screen -> k_mi_units, the only path.  1 (the fused GEMM + MI epilogue kernel: 132 against 122 ms per
 * C4 step) has been removed and answers LDW_ERR_STATE. */
int ldw_set_fused(ldw_ctx *ctx, int on);
/* Mixed precision (default on; 5 weight limbs, two-kernel path, speculative blocks): the block-wide co-occurrence GEMM runs
 * with the 3 HIGH limbs of the fixed-point weights only — all the fp32 screen needs; its margin is widened by a rigorous
 * bound of what the low limbs can add — and the exact joint sums of the units the screen lists (3-4 % of an off-diagonal
 * block, the short-range band of a diagonal one) get their 2 low limbs from a gathered GEMM over just those rows:
 * sum = (high << 16) + low, the same integers as the 5-limb GEMM. */
int ldw_set_mixed(ldw_ctx *ctx, int on);
/* Which block-wide pass feeds the screen of the speculative blocks (every block but the first of a call sequence):
 * 0 (default) = the approximate-GEMM path when the weights allow it — ONE int8 MFMA pass with dual-digit block-floating-
 *     point weights (V ~ a b 2^e, rigorous relative error bound in the screen's margin), exact joint sums of the listed
 *     units by class-wise popcounts over the weight classes (sequences of equal weight are contiguous in the bit rows),
 *     exact re-screen, fp64 — else the limb paths; 1 = the limb paths of ldw_set_mixed only; 2 = the approximate path or
 *     LDW_ERR_STATE at block time when the weights do not allow it (too many distinct weights, > 30k sequences). */
int ldw_set_path(ldw_ctx *ctx, int mode);
/* Long-range selection of the speculative blocks: 0 (default) = without a sort where it applies (radix select of the threshold,
 * bitmap ranks over the row-order key space: ldw_mi.hip k_sel_*), 1 = always the general path (two radix sorts). */
int ldw_set_select(ldw_ctx *ctx, int mode);
/* fp32 screen in front of the fp64 MI evaluation, in blocks that run the speculative selection: a long-range pair
 * only matters if its MI reaches the guessed histogram bucket, so MI is first bounded in fp32 (v_log_f32, proven
 * error < 1.3e-5 nats, margin 2e-4) and the exact value is computed for the waves that hold a pair which may pass, or a
 * short-range pair.  0 = off, 1 = on (default), 2 = verify: evaluate everything both ways and count lost pairs in
 * ldw_ctx_counters[3]. */
int ldw_set_screen(ldw_ctx *ctx, int mode);
/* Tile pruning of the approximate path (default on; LDW_NO_PRUNE in the environment = off).  In a block pair without a short-range
 * pair the order of the rows within a slot class is free, so the biallelic SNPs are ordered by the weight of their minor state;
 * a 128 x 64 wave tile of the approximate GEMM whose rectangle of threshold-table bins holds only unconditional entries — no joint
 * count can lift a pair of such marginals to the block's level; real alignments are full of near-singleton sites — is then
 * flagged clean without being computed or screened.  The same table entries dismiss the same pairs either way; verify mode
 * (ldw_set_screen 2) checks the pruned tiles' pairs in fp64 like every other dismissal. */
int ldw_set_prune(ldw_ctx *ctx, int on);
/* (test hook) a fixed capacity for the pair lists of the approximate path (0: automatic) — a list that overflows makes its block fall
 * back like a wrong guess; process-wide. */
int ldw_set_pair_cap(uint32_t cap);
/* Forget what earlier passes of this context learnt about the workload — the per-kind histogram-bucket guesses of the long-range
 * threshold, their spread history and the biallelic threshold table — without touching the alignment, the weights or any
 * buffer.  The next ldw_mi_all_pairs then runs as the FIRST pass of a job does (the reference visits every block pair once,
 * R/computePairwiseMI.R:103-116); bench.py calls it before every timed step.  Results never depend on this state. */
int ldw_reset_speculation(ldw_ctx *ctx);

/* ---- reports of the all-pairs loop ----------------------------------------------------------------------------------------- */
/* Which execution path the blocks of this context took since it was created (a real data set may fail a gate silently):
 * out[0] blocks through the approximate-GEMM path, out[1] through the mixed-precision limb path, out[2] through the plain path
 * (5-limb GEMM + fp64 MI of every pair: blocks without a bucket guess and every block when neither fast path applies),
 * out[3] = 0 (was: the removed fused kernel), out[4] speculation misses (blocks redone non-speculatively), out[5] blocks whose guess came from
 * the sampled probe of the block itself (cold starts), out[6] pairs listed for exact evaluation, out[7] units listed.
 * gate (capacity bytes, may be NULL) receives a short text: "ok" ("ok (block exponents per 32 positions)" when the weights'
 * dynamic range needs the finer exponents) or which gate keeps the approximate path off
 * ("delta 5.1e-03 > 4e-03", "Npad 40960 > 30720", "popcount segment tables 70000 B > 60000 B of LDS", "weights not set"). */
int ldw_path_report(ldw_ctx *ctx, int64_t out[8], char *gate, int capacity);
/* Kernel launches by form since the context was created, so that a test can tell which form of a size-dependent stage ran (results do not
 * depend on the form): the exact pair sums of the approximate path's listed pairs (ldw_pairs.hip; the form is choose_pair_form's, ldw_pairs.h), two launches per block, out[0] walking the set bits against
 * a per-position weight table within the default 64 KB of LDS (k_pair_sums_bits), out[1] the same with the 160-KB dynamic-LDS attribute
 * (more than 8 192 padded sequences), out[2] class-wise popcounts with the segment tables in LDS (k_pair_sums_q, or k_pair_sums under
 * LDW_PAIR_WAVE=1), out[3] the same with the tables in global memory (k_pair_sums: many weight classes beyond the bit walk's 160 KB, or LDW_NO_PAIR_BITS set); out[4] launches of the bit-row fill that
 * reads the states from global memory instead of staging a row in LDS (more than 61 440 padded sequences). */
int ldw_pair_form_report(ldw_ctx *ctx, int64_t out[5]);
/* Launches of the class-wise pair sums (out[2] + out[3] above; kernels of ldw_pairs.hip) by kernel since the context was created: out[0] the kernel with a quarter-wave
 * per pair and persistent waves (the default where the segment tables fit LDS), out[1] the kernel with a wave per pair (tables in global
 * memory, or LDW_PAIR_WAVE=1, read per call).  Both give the same sums. */
int ldw_pair_kernel_report(ldw_ctx *ctx, int64_t out[2]);
/* tile pruning (ldw_set_prune): out[0] blocks whose rows were ordered, out[1] wave tiles pruned, out[2] wave tiles of the GEMMs that
 * could prune (both since the context was created; pruned tiles are not counted as executed work by ldw_gemm_stats), out[3] = on. */
int ldw_prune_report(ldw_ctx *ctx, int64_t out[4]);
/* spans (ldw_set_span): out[0] spans run, out[1] reference blocks they covered, out[2] segments redone on their own after a wrong guess,
 * out[3] on. */
int ldw_span_report(ldw_ctx *ctx, int64_t out[4]);
/* List overflows.  The default path lists its candidates in fixed-capacity device lists; a list that overflows makes its block (or
 * its segment of a span) be redone on the plain path (counted in spec_misses like a wrong bucket guess), so results never depend on a
 * capacity.  out[0] blocks / segments redone because a PAIR list overflowed, out[1] because the MAYBE list of the approximate GEMM's
 * epilogue did (sized for the worst case: non-zero only under the test override LDW_MAYBE_CAP), out[2] = 1 while the maybe list
 * is switched off for the rest of the pass after such an overflow (ldw_reset_speculation switches it on again), out[3] entries handed to the
 * maybe list since the context was created. */
int ldw_overflow_report(ldw_ctx *ctx, int64_t out[4]);
/* The per-slot device buffers of a block's launch chain (csrc/ldw_slots.h): out[0] reallocations since the context was created — a buffer that
 * had to grow where it is used, or that ldw_ctx_reserve had not made —, out[1..5] bytes held now, summed over the pipeline slots, by the unit
 * lists, the per-block SNP constants, the pair lists, the row bins / flags and the maybe list's extracts. */
int ldw_slot_report(ldw_ctx *ctx, int64_t out[6]);
/* What the library holds on the GPU side, process-wide (all devices, all contexts): out[0] device blocks held by live buffers, out[1] released
 * device blocks waiting on the free list (ldw_host_trim empties it), out[2] pinned host blocks, out[3] events, out[4] streams the library
 * created and has not destroyed (a stream handed in by ldw_ctx_set_stream is never counted).  A context's share of out[0], out[2], out[3] and
 * out[4] is gone after ldw_ctx_destroy: tests/test_ctx_lifecycle_gpu.py compares the counts around whole jobs. */
int ldw_resource_report(int64_t out[5]);

/* ---- inspection and test hooks (BOUNDS.md; tests/test_bounds.py brute-forces every bound of the default path through them;
 *      ldweaver_amd/csrc/ldw_debug.hip) ------------------------------------------------------------------------------------------- */
/* the per-SNP bounds behind the pruning of the 2 x 3 / 3 x 3 tables.  out[a * 4 + 2 * m + (k - 2)] = the largest MI
 * SNP a (2 or 3 states, all flagged in uqe, r = its number of states) can reach with ANY partner that has k = 2 or 3 flagged states
 * and r = k — the maximum of the MI over the joint tables with a's marginals, which is convex there and sits at a vertex: every
 * state of a sends all its weight to one state of the partner — under the intended (m = 0) and the reference (m = 1: RXY at its
 * floor min(r)^2 / 4) reading of RXY; 1e300 for other SNPs and for SNPs with a sizeable minor state (not evaluated).  Needs the
 * alignment, the weights and the SNP meta data; capacity in doubles (>= 4 L). */
int ldw_snp_bounds(ldw_ctx *ctx, double *out, int64_t capacity);
/* out[0] = pairs that verify mode (ldw_set_screen 2) counted as "the screen would have lost this one" since the last call, out[1 + 4 k ..]
 * = (from SNP, to SNP, exact MI, level) of the first 16 of them.  65 doubles. */
int ldw_debug_violations(ldw_ctx *ctx, double *out);
/* the threshold table of the biallelic pairs (k_build_tab11) for a total weight W, an MI level lo, the approximate sums' relative
 * error delta, their absolute slack eta and the unit sprime of the int32 sums: out[64 * 64 * 2] = (Lq, Hq) of entry [bin of the to side][bin of the
 * from side], bin = min(63, floor(sqrtf(p) * cbin)); a sum n' with Lq < n' < Hq is dismissed.  tests/test_gpu_parity.py checks the table against
 * the MI formula on a grid of joint tables. */
int ldw_debug_tab11(ldw_ctx *ctx, double W, double lo, double delta, double eta, double sprime, int32_t *out, double *cbin_out);
/* ldw_debug_apx_params: the constants the approximate screen's bound is built from for the CURRENT weights, as the engine derives them:
 *   out[0] F (fraction bits of the fixed-point weights), [1] e_last, [2] delta = max |V'/V - 1|, [3] lost units of a GEMM entry, [4] sum of the fixed-point weights,
 *   [5] neff, [6] apx_EG, [7] apx_dfac, [8] apx_s1, [9] apx_c1, [10] apx_W, [11] apx_unit = 2^(e_last - F), [12] scr_scale of the approximate screen,
 *   [13] scr_shift and [14] scr_scale of the exact-limb screen, [15] bit 0: the path is usable, bit 1: block exponents per 32 positions,
 *   [16] lo_abs_sum = sum |V_lo| 2^-F and [17] lo_bound, the margin the mixed-precision screen adds for the two low limbs, [18] apx_MU (units a floor marginal can be low: 1, or 0 at e_last = 0), [19] limbs;
 *   vfixed_out / vapx_out (may be NULL; capacity >= N): the exact fixed-point weight V_s and its dual-digit approximation V'_s = a b 2^e of every SEQUENCE.
 * ldw_debug_rows: row0_out[L + 1] = first indicator row of every SNP, slot_meta_out[L] = rows (3 bits) | uqe flag of slot i << (3 + i) | state of slot i << (8 + 3 i).
 * ldw_debug_apx_gemm: gemm_apx_kernel over the given indicator rows (indices 0..R; R = the all-zero padding row): out[nrt][nrf] = the int32 sums G' in units of 2^e_last.
 * ldw_debug_apx_gemm_list: the same contract and the same values through the kernel's LIST launch (the default path's, without its table test): a list of every
 *   wave tile (128 to-rows x 64 from-rows) that holds an entry of out, walked by grid_wgs workgroups (1..65536) of four waves — wave w takes the tiles w, w + 4 grid_wgs,
 *   ... of the list; workgroups beyond the list leave at once.
 * ldw_debug_apx_gemm_fused: the approximate GEMM as the default path launches it — FUSED with the threshold-table test of its epilogue (clean-region flags, maybe list) and,
 *   with prune != 0, behind the live-tile pass (tile-pruning rules (a) and (b)) — through the product's own launch code, unchanged: launch_pack_panel, launch_apx_live_tiles,
 *   launch_gemm_apx with fuse = 1, on caller-made inputs.  rows_t[nrt] / rows_f[nrf] (1..8192 each): as for ldw_debug_apx_gemm, padded with R to multiples of 128 (RTpad, RFpad).
 *   bin_t[nrt] / bin_f[nrf]: the table bin 0..63 of every row, or 255 (no bin); padding rows get 255, as k_build_packs leaves them.  rflag_t[nrt] / rflag_f[nrf] (both or neither
 *   NULL): the pruning flags of every row (kind 2 or 3 in bits 0-1, 4 = dead versus kind 2, 8 = dead versus kind 3), read by the live-tile pass only; padding rows get 0.
 *   tab[64 * 64 * 2]: int32 (Lq, Hq) of entry [bin_t][bin_f], the caller's own (a sum n' with Lq < n' < Hq passes).  sr_mask (may be NULL): [RTpad / 128][RFpad / 64] bytes, != 0 =
 *   the tile is never table-tested.  lower_only: a diagonal block's launch (tiles with tx * 64 + 63 < ty * 128 are no part of it).  prune = 0: the 2-D launch; prune != 0: the
 *   live-tile pass, then the list launch with grid_wgs workgroups (1..65536; 0 = apx_run_grid's; without prune grid_wgs must be 0).  maybe_cap: -1 = no maybe list, else its
 *   capacity 1..1 048 576.  Every output is the raw device buffer, filled with bytes LDW_DEBUG_APX_FUSED_FILL before the launches — the clean flags too, which the product zeroes:
 *   what no kernel wrote still holds the pattern.  G_out[RTpad][RFpad] int32: the stored regions (32 to-rows x 64 from-rows each); clean_out[RTpad / 32][RFpad / 64]: the region
 *   flags; tiles_out[(RTpad / 128) * (RFpad / 64)] (prune only, else may be NULL): the live-tile list, ty * (RFpad / 64) + tx; maybe_out[maybe_cap][3] (may be NULL without a list):
 *   (to-row position, from-row position, n') of the entries handed over; counts_out[4]: live tiles, tiles the live-tile pass counted as pruned (a counter of the hook's own), the
 *   final count of the maybe list (it counts beyond the capacity), and the bytes written behind the list's capacity (a guard of 64 entries on the device: 0).  A live tile's region with no row or column of bin 255 and no mask is flagged 1 and not stored when every
 *   entry passes, or when a maybe list is given and at most LDW_DEBUG_APX_MAYBE_MAX entries fail (those go to the list); every other region of a live tile is flagged 0 and stored.
 *   LDW_ERR_STATE: the weights do not allow the approximate path; LDW_ERR_ARG: a row outside 0..R, a bin in 64..254, counts outside 1..8192, grid_wgs != 0 without prune or outside
 *   0..65536, maybe_cap outside -1, 1..1 048 576, the flags of one side only.  Nothing is launched then and no output is written; the counters of ldw_gemm_stats and ldw_prune_report
 *   never move, refused or not.  tests/test_apx_fused_gpu.py compares every flag, stored integer, list entry and count with the plain-loop model of tests/apx_fused_ref.py;
 *   tests/apx_fused_cases.py makes the cases and tests/test_apx_fused_cases_host.py checks without a GPU that they hold the situations they were made for.
 * ldw_debug_limb_gemm: the exact co-occurrence GEMMs as functions: launch_gemm_bits (engine 0: gemm_bits_kernel<J>) or launch_cooc_popc (engine 1: k_cooc_popc), unchanged, over
 *   caller-given indicator rows of the context's current bit rows and weights.  rows_t[nrt] / rows_f[nrf] (1..8192 each): row indices 0..R, R = the all-zero padding row; both
 *   lists are padded to multiples of 128 with R (RTpad, RFpad).  Engine 0: the launch gets the digit limbs limb0 .. limb0 + nlimbs - 1 of the weights (digits + limb0 * Kpad, as
 *   the mixed path asks for its three high limbs), nlimbs in 1..6 (six run as 3 + 3: the second launch shifts by 24 bits and accumulates), limb0 >= 0 and limb0 + nlimbs <= the
 *   limb count of ldw_set_weights; lower_only: the launch of a diagonal block (tiles of 128 to-rows x 64 from-rows with bx * 64 + 63 < by * 128 are left out); by0, by1: the strip
 *   of tile rows by0 <= by < by1 (by1 < 0: all RTpad / 128); tile_mask (may be NULL): [RTpad / 128][RFpad / 64] bytes, 0 = the tile is left out; tile_list (may be NULL) with
 *   n_tile_list entries by << 16 | bx (by < RTpad / 128, bx < RFpad / 64; at most 65 536): a 1-D launch over exactly these tiles, whatever lower_only and the mask say — the engine
 *   passes the mask with the list, so both may be given; n_tile_list = 0 is a legal launch of nothing (LDW_OK); a list needs by0 = 0.  Engine 1 takes limb0 = 0, all the limbs,
 *   no mask, no list and no strip; its lower_only rule is on tiles of 64 x 64 rows (tx * 64 + 63 < ty * 64 is left out).  out[nrt][nrf] int64:
 *   out[t][f] = sum over the sequences s of V_part(s) [row t has s][row f has s],  V_part = sum_j d_(limb0 + j) 256^j  over the balanced base-256 digits d of the fixed-point weight.
 *   The device buffer is filled with bytes LDW_DEBUG_LIMB_GEMM_FILL before the launch: every int64 no kernel wrote still holds that pattern.
 *   LDW_ERR_STATE: no weights set (engine 1: no popcount segments); LDW_ERR_ARG: engine outside 0..1, a row outside 0..R, nrt / nrf outside 1..8192, nlimbs outside 1..6, limbs
 *   beyond the context's, by0 >= by1 or a strip outside the tile rows, a list with by0 != 0, more than 65 536 entries or a tile outside the grid, n_tile_list != 0 without a list.
 *   Nothing is launched then and out is not written; the counters of ldw_gemm_stats never move, refused or not.  tests/test_limb_gemm_fn_gpu.py compares every stored integer
 *   with the integer sums of numpy.
 * ldw_debug_lo_units: the gathered low-limb GEMM of the mixed path (launch_gemm_lo_units: gemm_lo_units_kernel) on caller-made unit lists.  from_snps[64 * ntiles] (ntiles in
 *   1..4096): the from-side SNPs in epilogue order, tile t = entries 64 t .. 64 t + 63, -1 = a padding lane; to_snps[nt] (nt in 1..1 048 576): any SNPs 0..L-1, repeats allowed:
 *   column slot q stands for to_snps[q].  counts[ntiles][3]: listed units per (tile, row-slot class lc = 0, 1, 2 for SNPs of <= 1, 2, >= 3 indicator rows); slots[]: the listed
 *   column slots of every (tile, lc) one list behind the other, tiles outermost (sum of counts entries).  A slot listed under lc must hold a SNP of that class, and a (tile, lc)
 *   lists at most as many units as to_snps holds SNPs of the class (the capacity of its rows).  The geometry is made by lo_layout (csrc/ldw_lo_geom.h), the function prep_block
 *   lays a block out with: geom_out[8] = rowbase[3], uoff[3], RTlo, (tile, fs) pairs of the launch; cmax_out[ntiles] = 1, 2, 4: slots per from-side SNP of the tile;
 *   tile_base_out[ntiles]: first int of the tile's block in glo; *glo_total_out: ints of glo.  glo_out == NULL: the geometry alone, nothing is launched.  Else glo_out[glo_capacity],
 *   glo_capacity >= glo total: the raw buffer, filled with bytes LDW_DEBUG_LO_UNITS_FILL before the launch.  For unit k of (tile, lc) — column slot q = its k-th listed slot — row j
 *   of SNP to_snps[q] and slot i of the SNP in lane ln of the tile, the int32 at tile_base[tile] + (rowbase[lc] + (k << lc) + j) * 64 cmax + ln * cmax + i is
 *   sum_s (d_0(s) + 256 d_1(s)) [to row has s][from row has s]; absent rows, absent slots and padding lanes give 0; the rows of a chunk of 128 beyond the last listed unit are
 *   written as 0; chunks no list reaches keep the fill.  Needs weights of at least two limbs (LDW_ERR_STATE) and at most 65 535 (tile, fs) pairs; LDW_ERR_ARG for SNPs, slots or
 *   counts outside these bounds and for a buffer above 2^28 ints; nothing is launched then.
 * ldw_debug_pair_sums: the exact joint sums of caller-made pair lists, by the sum kernels alone (no MI, no emission) and through the launch code of the default path (launch_pair_sums, ldw_pairs.hip).
 *   The lists are those of the approximate screen: 5 paths x 8 shards, list = path * 8 + shard, paths 0..3 for SNP pairs of (1,1), (2,1), (1,2), (2,2) indicator rows
 *   (from side, to side), path 4 for any 1..4 x 1..4.  counts[40] = entries of every list (a count above cap is clamped by the kernels, as after an overflow);
 *   snp_a / snp_b[40][cap] = the SNPs of the entries (from side, to side), read up to min(count, cap) per list.  form: 0 = what the default path would launch, 1 = a
 *   quarter-wave per pair (k_pair_sums_q), 2 / 3 = a wave per pair with the segment tables in LDS / in global memory (k_pair_sums), 4 = the bit walk
 *   (k_pair_sums_bits); *form_out (may be NULL) = the form that ran.  grid_wgs: 0 = the default path's grid, else (1..65536) gridDim.x of both launches — the whole
 *   grid of a path for form 1 (wave w of the 4 grid_wgs waves takes the groups of four pairs w, w + 4 grid_wgs, ... of the path's eight shards walked as one index
 *   space), workgroups per list for the others.  sums_out[40][cap][16] int64: entry j * 4 + i of a pair = sum over the sequences of the fixed-point weight where
 *   SNP a is in the state of its row i and SNP b in that of its row j; paths 0..3 write the rows x rows entries k_pair_mi reads, path 4 all sixteen (0 for an absent
 *   row).  The buffer is filled with bytes LDW_DEBUG_PAIR_SUMS_FILL before the launches: every int64 the kernels did not write still holds that pattern.
 *   LDW_ERR_STATE: no weights set, or a forced form cannot run (forms 1, 2: the segment tables exceed 60 000 B of LDS; form 4: the per-position table exceeds
 *   160 KB); LDW_ERR_ARG: cap outside 1..65536, an SNP outside 0..L-1, row counts that are not the list's.  Nothing is launched then, and no launch counter
 *   (ldw_pair_form_report, ldw_pair_kernel_report) ever moves.  tests/test_pair_sums_fn_gpu.py compares every form with the integer sums of numpy.
 * ldw_debug_screen_bound: the engine's own device functions on n caller-made joint tables (arrays by case: g[16] = sums of the indicator rows, g[j * 4 + i] = slot i of the
 *   from-side SNP x slot j of the to-side SNP; pa / pb[5] integer marginals by slot; pX / pY[5] weighted marginals; rr[3] = r_a, r_b, RXY; masks[2] = slot meta of both SNPs,
 *   kinds 1 / 3 only; params = the 20 numbers of ldw_debug_apx_params, which the caller may alter).  kind 0: full_cells_screen<na, nb, APX> — the approximate path's upper
 *   bound of MI; 1: pair_screen_generic<APX>; 2: full_cells_screen<na, nb> on exact sums (an fp32 MI); 3: pair_screen_generic on exact sums; 4: full_cells_mi<na, nb>, the
 *   fp64 value the engine emits (out64).  na, nb in {1, 2} for kinds 0 / 2 / 4. */
int ldw_debug_apx_params(ldw_ctx *ctx, double out[20], int64_t *vfixed_out, int64_t *vapx_out, int64_t capacity);
int ldw_debug_rows(ldw_ctx *ctx, int32_t *row0_out, uint32_t *slot_meta_out, int64_t capacity);
int ldw_debug_apx_gemm(ldw_ctx *ctx, const int32_t *rows_t, int nrt, const int32_t *rows_f, int nrf, int32_t *out);
int ldw_debug_apx_gemm_list(ldw_ctx *ctx, const int32_t *rows_t, int nrt, const int32_t *rows_f, int nrf, int grid_wgs, int32_t *out);
#define LDW_DEBUG_APX_FUSED_FILL 0xA5 /* every byte of G_out, clean_out, tiles_out and maybe_out no kernel wrote */
#define LDW_DEBUG_APX_MAYBE_MAX 96    /* the build's APX_MAYBE_MAX: most failing entries of a region that go to the maybe list */
int ldw_debug_apx_gemm_fused(ldw_ctx *ctx, const int32_t *rows_t, int nrt, const int32_t *rows_f, int nrf, const uint8_t *bin_t, const uint8_t *bin_f, const uint8_t *rflag_t,
                             const uint8_t *rflag_f, const int32_t *tab, const uint8_t *sr_mask, int lower_only, int prune, int grid_wgs, int maybe_cap, int32_t *G_out,
                             uint8_t *clean_out, uint32_t *tiles_out, int32_t *maybe_out, int64_t counts_out[4]);
#define LDW_DEBUG_LIMB_GEMM_FILL 0xA5 /* every byte of out no kernel wrote */
int ldw_debug_limb_gemm(ldw_ctx *ctx, int engine, const int32_t *rows_t, int nrt, const int32_t *rows_f, int nrf, int limb0, int nlimbs, int lower_only, int by0, int by1,
                        const uint8_t *tile_mask, const uint32_t *tile_list, int n_tile_list, int64_t *out);
#define LDW_DEBUG_LO_UNITS_FILL 0xA5 /* every byte of glo_out the kernel did not write */
int ldw_debug_lo_units(ldw_ctx *ctx, const int32_t *from_snps, int ntiles, const int32_t *to_snps, int nt, const uint32_t *counts, const int32_t *slots, int32_t geom_out[8],
                       int32_t *cmax_out, int64_t *tile_base_out, int64_t *glo_total_out, int32_t *glo_out, int64_t glo_capacity);
#define LDW_DEBUG_PAIR_SUMS_FILL 0xA5 /* every byte of sums_out the kernels did not write */
int ldw_debug_pair_sums(ldw_ctx *ctx, int form, int grid_wgs, uint32_t cap, const uint32_t *counts, const int32_t *snp_a, const int32_t *snp_b, int64_t *sums_out,
                        int *form_out);
int ldw_debug_screen_bound(ldw_ctx *ctx, int kind, int na, int nb, int64_t n, const int64_t *g, const int64_t *pa, const int64_t *pb, const float *pX, const float *pY,
                           const double *rr, const uint32_t *masks, const double params[20], float *out, double *out64);

/* ---- LD decay (ldweaver_amd.h 20) --------------------------------------------------------------------------------------------------------------------------
 * ldw_debug_profile_hist: the histogram kernel of ldw_mi_profile (k_decay_hist) as a function, on caller-made values; needs no alignment.  mi[nf * nt]
 *   (HOST, column-major: the pair (a_loc, b_loc) at a_loc + b_loc * nf; no NaN), pos_f[nf] / pos_t[nt] the positions of the two sides, g > 0 the genome
 *   length, diag = 1 (nf == nt): the pairs a_loc > b_loc, diag = 0: the pairs a_loc != b_loc; cuts, n_cut, mi_shift and the three outputs as ldw_mi_profile.
 *   The kernel works in patches of 64 rows x 256 columns; a patch bounds its distance bins lo..hi from the extreme positions of its rows and columns and
 *   counts in LDS when (hi - lo + 1) * NB <= 8192 counters fit (route A), else by wave-aggregated global adds (route B).  route: 0 = every patch chooses,
 *   1 = route A, LDW_ERR_ARG (outputs undefined) when a patch does not fit, 2 = route B for every patch.  All give the same bytes.  stats_out (may be NULL,
 *   3 values): patches with a pair, patches that took route B, pairs found outside their patch's bound (added one by one; 0 for integral g).
 *   LDW_ERR_ARG: nf, nt outside 1..1 000 000, diag with nf != nt, g not positive, route outside 0..2, cuts or mi_shift as ldw_mi_profile refuses them.
 * ldw_decay_report: out[0..2] the same three counts summed over the last ldw_mi_profile of the context, out[3] its blocks. */
int ldw_debug_profile_hist(ldw_ctx *ctx, const double *mi, int64_t nf, int64_t nt, const int32_t *pos_f, const int32_t *pos_t, double g, int diag,
                           const double *cuts, int32_t n_cut, int32_t mi_shift, int route, uint64_t *hist_out, double *max_out, int64_t *npairs_out,
                           int64_t *stats_out);
int ldw_decay_report(ldw_ctx *ctx, int64_t out[4]);

/* ---- per-SNP MI summary (ldweaver_amd.h 21) ------------------------------------------------------------------------------------------------------------------
 * ldw_debug_snp_summary: the kernel of ldw_mi_snp_summary (k_snp_summary) as a function, on caller-made values; needs no alignment.  mi, nf, nt, pos_f, pos_t,
 *   g and diag as ldw_debug_profile_hist (mi may hold any double, NaN included); sr_dist and thr[2] as ldw_mi_snp_summary.  The two sides come out apart:
 *   n_f / sumq_f / max_f / nge_f [2][nf] what the pairs add to their from-SNPs (the rows), n_t / sumq_t / max_t / nge_t [2][nt] what they add to their to-SNPs
 *   (the columns); max_* and nge_* may be NULL.  npairs_out[2] the pairs of each class.
 *   The kernel works in patches of 64 rows x 256 columns; a patch bounds its distances from the extreme positions of its rows and columns.  route: 0 = a patch
 *   the bound puts in one class carries one set of accumulators (route 1), any other both (route 2); 1 = route 1, LDW_ERR_ARG (outputs undefined) when the
 *   bound does not put a patch in one class; 2 = route 2 for every patch.  All give the same integers.  stats_out (may be NULL, 4 values): patches
 *   visited (every patch but a diagonal block's patches that lie wholly on or above the diagonal; a visited patch may hold no pair), patches on route 2, pairs whose own class is not their route-1 patch's (added one by one), values q refused (once per pair).
 *   LDW_ERR_ARG: nf, nt outside 1..1 000 000, diag with nf != nt, g not positive, route outside 0..2, sr_dist negative or NaN.
 * ldw_snp_summary_report: out[0..3] the same four counts summed over the last ldw_mi_snp_summary of the context, out[4] its blocks. */
int ldw_debug_snp_summary(ldw_ctx *ctx, const double *mi, int64_t nf, int64_t nt, const int32_t *pos_f, const int32_t *pos_t, double g, int diag, double sr_dist,
                          const double *thr, int route, int64_t *n_f, int64_t *sumq_f, double *max_f, int64_t *nge_f, int64_t *n_t, int64_t *sumq_t, double *max_t,
                          int64_t *nge_t, int64_t *npairs_out, int64_t *stats_out);
int ldw_snp_summary_report(ldw_ctx *ctx, int64_t out[5]);

/* ---- selection by a corrected score (ldweaver_amd.h 22) ------------------------------------------------------------------------------------------------------
 * ldw_debug_score_scan / ldw_debug_score_links: the kernels of ldw_mi_score_scan (k_score_scan) and ldw_mi_score_links (k_score_links) as functions, on
 *   caller-made values; they need no alignment.  mi, nf, nt, pos_f, pos_t, g and diag as ldw_debug_snp_summary (mi may hold any double); sr_dist and cls_mask
 *   as (22); w_f[nf] / w_t[nt] the weights of the two sides, finite.  The two sides come out apart.
 *   scan: hist_out[4096], best_f[nf] / best_t[nt] the largest score of every row / column (NaN: none), *npairs_out the pairs inside the mask.
 *   links: id_f[nf] / id_t[nt] the global ids of the two sides, 0..2^31 - 2, in any order (the scan needs none); thr, cap, the four lists (a_out from id_f,
 *   b_out from id_t) and *count_out as (22); best_f / best_t (both or neither) and partner_f[nf] / partner_t[nt] (both or neither, they need the bests): per
 *   row the smallest id_t among its partners whose score has the key of best_f, per column the smallest id_f likewise; -1: none.
 *   stats_out (may be NULL, 2 values): patches visited (every patch but a diagonal block's patches that lie wholly on or above the diagonal), NaN scores.
 *   LDW_ERR_ARG: nf, nt outside 1..1 000 000, diag with nf != nt, g not positive, what (22) refuses, an id outside its range.
 * ldw_score_select_report: out[0..1] the same two counts summed over the last ldw_mi_score_scan or ldw_mi_score_links of the context, out[2] its blocks. */
int ldw_debug_score_scan(ldw_ctx *ctx, const double *mi, int64_t nf, int64_t nt, const int32_t *pos_f, const int32_t *pos_t, double g, int diag, double sr_dist,
                         int cls_mask, const double *w_f, const double *w_t, uint64_t *hist_out, double *best_f, double *best_t, int64_t *npairs_out,
                         int64_t *stats_out);
int ldw_debug_score_links(ldw_ctx *ctx, const double *mi, int64_t nf, int64_t nt, const int32_t *pos_f, const int32_t *pos_t, double g, int diag, double sr_dist,
                          int cls_mask, const int32_t *id_f, const int32_t *id_t, const double *w_f, const double *w_t, double thr, const double *best_f,
                          const double *best_t, int64_t cap, int32_t *a_out, int32_t *b_out, double *mi_out, double *score_out, int64_t *count_out,
                          int32_t *partner_f, int32_t *partner_t, int64_t *stats_out);
int ldw_score_select_report(ldw_ctx *ctx, int64_t out[3]);

/* ---- the co-change scan (ldweaver_amd.h 23) ------------------------------------------------------------------------------------------------------------------
 * ldw_debug_cochange_scan / ldw_debug_cochange_links: the pair kernel of ldw_tree_cochange_scan and ldw_tree_cochange_links (k_coscan) as functions, on
 *   caller-made bitmaps; they need no alignment and no tree, and run the launch code of the two entries (bands, LDW_COSCAN_ROWS, initialisation).  All from the
 *   HOST: bits[words][M] (word w of slot s at bits[w M + s]; any bits, words 1..2^16), M in 0..2^24 slots standing for the eligible SNPs; changes[M] what the
 *   lift test multiplies (0..2^21 - 1; the entries do not require the popcount of the row); idx[M] the global SNP of every slot, strictly ascending, 0..2^31 - 2;
 *   pos[M] and g (needed where min_len >= 0); B in 1..2^21 - 1; min_co, min_lift, min_len as (23).  The pair set, the qualifying pairs and every output are
 *   those of (23) over the M slots: hist_out[1024], best_out[M], nge_out[M], npairs_out[2]; best_in[M], cap, the three lists (global SNPs from idx), *count_out
 *   and partner_out[M] (a global SNP, or -1).  LDW_ERR_ARG: what (23) refuses of the thresholds and of the lists, a size or a value outside the ranges above,
 *   idx not ascending, a null pointer among those M > 0 needs. */
int ldw_debug_cochange_scan(ldw_ctx *ctx, const uint32_t *bits, int64_t words, int64_t M, const int32_t *changes, const int32_t *idx, const int32_t *pos, double g,
                            int64_t B, int32_t min_co, int64_t min_lift, double min_len, uint64_t *hist_out, int32_t *best_out, int64_t *nge_out,
                            int64_t *npairs_out);
int ldw_debug_cochange_links(ldw_ctx *ctx, const uint32_t *bits, int64_t words, int64_t M, const int32_t *changes, const int32_t *idx, const int32_t *pos, double g,
                             int64_t B, int32_t min_co, int64_t min_lift, double min_len, const int32_t *best_in, int64_t cap, int32_t *a_out, int32_t *b_out,
                             int32_t *co_out, int64_t *count_out, int32_t *partner_out);

/* ---- the segment map (ldweaver_amd.h 24) ---------------------------------------------------------------------------------------------------------------------
 * ldw_debug_segment_map / ldw_debug_segment_best: the kernels of ldw_mi_segment_map and ldw_mi_segment_best (k_segment) as functions, on caller-made values;
 *   they need no alignment.  mi, nf, nt, pos_f, pos_t, g and diag as ldw_debug_snp_summary (mi may hold any double); seg_f[nf] / seg_t[nt] the segments of the
 *   two sides, S, sr_dist, cls_mask and thr as (24); w_f[nf] / w_t[nt] the weights of the two sides, finite, both or neither.  The outputs are those of (24).
 *   best: id_f[nf] / id_t[nt] the global ids of the two sides, 0..2^31 - 2, in any order; max_in[S * S] and pair_out[S * S] as (24), packed from the ids.
 *   The kernel works in patches of 64 rows x 256 columns and cuts the segment ids of a patch's rows and columns into runs.  route: 0 = a patch of at most 8
 *   row runs and 16 column runs keeps a window of cells in LDS (route 1), any other adds per pair, the lanes of a cell combined (route 2); 1 = route 1,
 *   LDW_ERR_ARG (outputs undefined) when a patch does not fit; 2 = route 2 for every patch.  All give the same bytes.  stats_out (may be NULL, 4 values): patches
 *   visited (every patch but a diagonal block's patches that lie wholly on or above the diagonal), patches on route 2, values q refused (map only; NaN
 *   included), NaN values.
 *   LDW_ERR_ARG: nf, nt outside 1..1 000 000, diag with nf != nt, g not positive, route outside 0..2, one of w_f / w_t alone, what (24) refuses, an id outside
 *   its range.
 * ldw_segment_map_report: out[0..3] the same four counts summed over the last ldw_mi_segment_map or ldw_mi_segment_best of the context, out[4] its blocks. */
int ldw_debug_segment_map(ldw_ctx *ctx, const double *mi, int64_t nf, int64_t nt, const int32_t *pos_f, const int32_t *pos_t, double g, int diag,
                          const int32_t *seg_f, const int32_t *seg_t, int32_t S, double sr_dist, int cls_mask, const double *w_f, const double *w_t, double thr,
                          int route, int64_t *n_out, int64_t *nge_out, int64_t *sum_lo_out, int64_t *sum_hi_out, double *max_out, int64_t *npairs_out,
                          int64_t *stats_out);
int ldw_debug_segment_best(ldw_ctx *ctx, const double *mi, int64_t nf, int64_t nt, const int32_t *pos_f, const int32_t *pos_t, double g, int diag,
                           const int32_t *seg_f, const int32_t *seg_t, int32_t S, double sr_dist, int cls_mask, const int32_t *id_f, const int32_t *id_t,
                           const double *w_f, const double *w_t, const double *max_in, int route, uint64_t *pair_out, int64_t *stats_out);
int ldw_segment_map_report(ldw_ctx *ctx, int64_t out[5]);

/* ---- the plots (ldweaver_amd.h 12) ------------------------------------------------------------------------------------------------ */
/* The rasters of ldw_plot_scatter without the frame, for panels of W x H pixels each (any size >= 1): rgb_out[n_panels][H][W][3] (host).  Grid
 * lines lie at the ticks of ldw_plot_ticks for the data range and W / H.  stats_out (may be NULL, 8 doubles): x min, x max, y min, y max of
 * the kept rows (the hline included), srp lo, hi over the kept layer-1 rows (NaN: none), rows kept, rows dropped.  *scratch_bytes_out (may be
 * NULL): device memory the render needs beyond the caller's columns (and, when on_device = 0, beyond the chunk buffer of at most 26 MiB and
 * the row-order key's copy of the srp column).  ms_out (may be
 * NULL, 4 doubles): hip-event times of the statistics pass, the key-image clear, the centre pass and the disc + colour pass. */
int ldw_debug_plot_panels(ldw_ctx *ctx, const double *x, const double *y, const double *srp, const uint8_t *layer, const uint8_t *panel, int64_t n,
                          int on_device, const ldw_plot_opts *opts, int n_panels, int32_t W, int32_t H, uint8_t *rgb_out, double *stats_out,
                          int64_t *scratch_bytes_out, double *ms_out);
/* The panel of ldw_plot_xy without the frame, W x H pixels (1..8192 each way): rgb_out[H][W][3] (host).  Grid lines lie at the ticks of ldw_plot_ticks for the
 * data range and W / H.  stats_out (may be NULL, 6 doubles): x min, x max, y min, y max of the kept rows and finite line vertices, rows kept, rows dropped.
 * ms_out (may be NULL, 4 doubles): hip-event times of the statistics pass, the key-image clear, the centre + segment passes and the paint pass. */
int ldw_debug_plot_xy_panel(ldw_ctx *ctx, const double *x, const double *y, const uint8_t *cls, int64_t n, int on_device, const double *line_x,
                            const double *line_y, int64_t n_line, const ldw_plot_xy_opts *opts, int32_t W, int32_t H, uint8_t *rgb_out, double *stats_out,
                            double *ms_out);
/* Host only: the 2056 colours of the LD map's ramp (kind 0, rgb_out 2056 x 3) or the scatter gradient at t[n] (kind 1, rgb_out n x 3). */
int ldw_debug_plot_colours(int kind, const double *t, int64_t n, uint8_t *rgb_out);
/* The raw raster of ldw_plot_network, before the host draws over it: rgb_out[H][W][3] (host).  ms_out (may be NULL, 2 doubles): hip-event times of the binning
 * (boxes, counts, sums, lists) and of the shading. */
int ldw_debug_plot_capsules(ldw_ctx *ctx, const ldw_capsule *caps, int64_t n_caps, int32_t W, int32_t H, uint8_t *rgb_out, double *ms_out);
/* The raw raster of ldw_plot_tanglegram, before the host draws over it: the capsules, then the rectangles: rgb_out[H][W][3] (host).  ms_out (may be NULL, 3
 * doubles): hip-event times of the binning and the shading of the capsules and of the rectangle pass (copy of the list, owner image, colours). */
int ldw_debug_plot_marks(ldw_ctx *ctx, const ldw_capsule *caps, int64_t n_caps, const ldw_rect *rects, int64_t n_rects, int32_t W, int32_t H, uint8_t *rgb_out,
                         double *ms_out);
/* The raw canvas of ldw_plot_tree (ldweaver_amd.h 15), before the host draws over it: rgb_out[H][W][3] (host).  ms_out (may be NULL, 4 doubles): hip-event
 * times of the clear (coverage image and canvas), the bars (counts, sums, adds), the bands (lines, fill) and the colour pass over the panel. */
int ldw_debug_plot_tree(ldw_ctx *ctx, int32_t W, int32_t H, const int32_t *panel, const ldw_bar *bars, int64_t n_bars, uint32_t bar_rgb, const uint8_t *levels,
                        int64_t n_tips, const uint32_t *palette, const int32_t *band_rect, int32_t n_bands, uint8_t *rgb_out, double *ms_out);
/* The last ldw_links_grep of the context, out8: [0] the whole call, ms (host clock); [1] inside gzread, ms (host clock); [2] chunk copies, [3] line kernels
 * (k_tsv_count, scan), [4] k_tsv_starts + k_links_grep, ms (hip events, summed over the chunks); [5] chunks; [6] bytes searched; [7] rows kept. */
int ldw_links_grep_stats(ldw_ctx *ctx, double *out8);
/* The last ldw_tsv_read of the context, out10: [0] the whole call, ms (host clock); [1] inside gzread, ms (host clock); [2] chunk copies, [3] line kernels
 * (k_tsv_count, scan), [4] k_tsv_starts + k_tsv_parse, ms (hip events, summed over the chunks); [5] slow-cell conversion and patch, ms (host clock round its
 * copies and kernel); [6] chunks; [7] bytes parsed; [8] times the columns moved to a larger buffer since the context was made; [9] bytes of the two pinned
 * chunk buffers held now. */
int ldw_tsv_stats(ldw_ctx *ctx, double *out10);
/* Measurement only (same values): 0 = k_tsv_parse reads its rows by cached global loads, 1 = from an LDS-staged tile of the chunk. */
int ldw_tsv_set_variant(ldw_ctx *ctx, int variant);

#ifdef __cplusplus
}
#endif
#endif /* LDWEAVER_AMD_DEBUG_H */
