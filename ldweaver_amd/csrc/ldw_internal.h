// Internal declarations shared by the translation units of libldweaver_amd.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <atomic>
#include <chrono>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/ldweaver_amd.h"
#include "../../include/ldweaver_amd_debug.h"
#include "ldw_own.h"   // DevBuf, PinnedBuf, PinnedPair, Event, Stream: what a context holds on the GPU, each freed by its destructor

// Pipeline slots of the all-pairs loop: the block-wide kernels (GEMM stream) may run LDW_NSLOT - 1 blocks ahead of the block whose
// lists the main stream is evaluating; every per-block buffer exists once per slot (block b uses slot b % LDW_NSLOT).
#define LDW_NSLOT 3

// Variants measured slower than this code (fused GEMM + epilogue, corner spans, ...) are recorded in docs/HISTORY.md, not kept here.

namespace ldw {

void set_error(const char *fmt, ...);
int hip_fail(hipError_t e, const char *what, const char *file, int line);

#define LDW_HIP(call)                                                        \
    do {                                                                     \
        hipError_t e__ = (call);                                             \
        if (e__ != hipSuccess) return ldw::hip_fail(e__, #call, __FILE__, __LINE__); \
    } while (0)

#define LDW_REQUIRE(cond, code, ...)   \
    do {                               \
        if (!(cond)) {                 \
            ldw::set_error(__VA_ARGS__); \
            return (code);             \
        }                              \
    } while (0)

constexpr int TILE = 128;     // GEMM block tile (rows on both sides)
constexpr int KSTEP = 128;    // bytes of K (sequences) per pipeline stage
constexpr int NBINS = 4096;   // level-1 histogram bins of the lr quantile search

struct BlockStat {
    int64_t n_lr_total = 0, n_lr_kept = 0, n_sr = 0;
    double disc_thresh = 0;
};
// what the host knew / learnt about a block (LDW_BLOCK_TRACE=1 prints one line per block at ldw_links_end)
struct BlockTrace {
    int diag = 0, guess = -1, B_true = -1, margin = 0, path = 0 /* 0 plain, 1 mixed, 2 apx, 4 span */, missed = 0, probed = 0;
    long long n_cand = 0;
};


// The short-range model's device buffers (ldw_srp.hip) and the geometry of the last ldw_sr_len_quantiles call, which every later entry point of
// the model runs on.  Other units borrow some of the buffers as working memory between the model's calls: ldw_post.hip cnt and q,
// ldw_mi.hip seg and out, ldw_multi.cpp out.
struct SrModel {
    DevBuf pack, key, pack2, key2, pay, pay2, off, q, n, md, part, shape, cnt, tmp;
    DevBuf lower, cur, out, seg;   // the model over ranks (ldw_sr_tail_extract ...): per-group bounds, cursors, the extracted rows, block segments
    int S = 0, nclust = 0;         // set by ldw_sr_len_quantiles before anything launches
    double sr_dist = 0;
    bool same_geometry(int nclust_, int32_t S_) const { return nclust_ == nclust && S_ == S; }
};

// The links kept by ldw_sr_pvalues (rows of the short-range table) or ldw_lr_tukey (rows of the long-range one), the ARACNE pool that goes
// with them, and the ARACNE flags.  Whatever replaces a link table empties the kept set and the pool and drops the flags: invalidate(), called
// by ldw_links_import, ldw_links_load, ldw_set_positions, ldw_mi_all_pairs_multi's adoption of the assembled tables and, before it counts,
// ldw_sr_pvalues.  ldw_lr_tukey borrows ar_val, ar_val2 and ar_flags as working memory: it drops the flags when it starts (drop_flags) and
// adopts its counts when it is done; ldw_sr_reduced_import adopts likewise; ldw_sr_pool_build resets n_pool alone.
struct KeptLinks {
    DevBuf row, meta, srp;                 // int64 row of the table, uint32 clust_c | first_cluster << 8 | dup << 16, double srp_max
    DevBuf pool_a, pool_b, pool_mi;
    DevBuf ar_key, ar_val, ar_key2, ar_val2, ar_off, ar_flags;
    int64_t n_red = 0, n_pool = 0;
    bool from_lr = false;    // row indexes the long-range table (ldw_lr_tukey) instead of the short-range one
    bool ar_valid = false;   // ar_flags holds the ARACNE flags of the CURRENT kept links: set by ldw_aracne_device alone
    void drop_flags() { ar_valid = false; }
    void invalidate() { n_red = n_pool = 0, drop_flags(); }
    void adopt(int64_t n_red_, int64_t n_pool_, bool from_lr_) { n_red = n_red_, n_pool = n_pool_, from_lr = from_lr_, drop_flags(); }   // a new kept set and pool are in the buffers
    int reserve_red(size_t rows) {
        if (int rc = row.reserve(rows * 8)) return rc;
        if (int rc = meta.reserve(rows * 4)) return rc;
        return srp.reserve(rows * 8);
    }
    int reserve_pool(size_t rows) {
        if (int rc = pool_a.reserve(rows * 4)) return rc;
        if (int rc = pool_b.reserve(rows * 4)) return rc;
        return pool_mi.reserve(rows * 8);
    }
    int64_t red_capacity() const { return (int64_t)std::min(row.cap / 8, std::min(meta.cap / 4, srp.cap / 8)); }
    int64_t pool_capacity() const { return (int64_t)std::min(pool_a.cap / 4, std::min(pool_b.cap / 4, pool_mi.cap / 8)); }
};
// ---- Sub-states of the context, grouped by lifetime.  Each header says who writes the group and what drops it; the chain that ties them together
// ---- (which setter drops what) is ldw_ctx's member functions below and the table in DESIGN.md 27.

// The sequence weights in fixed point.  Written by ldw_set_weights alone; dropped by a new alignment shape (ldw_ctx::new_shape).
struct Weights {
    bool have_weights = false;
    int nlimbs = 5;
    int frac_bits = 0;
    double neff = 0;            // sum(hdw) like R's sum()
    int64_t total_fixed = 0;    // sum of quantised weights
    DevBuf digits;              // int8 [nlimbs][Npad] balanced base-256 digits of V_s
    DevBuf vfixed;              // int64 [Npad] quantised weights V_s (0 in the padding)
    std::vector<int64_t> h_vfixed;
    std::vector<double> h_hdw;  // [N] the weights as given (ldw_links_stratified sums them per cluster, by the rule of neff)
    // mixed-precision path (nlimbs == 5): V = V_hi * 2^16 + V_lo, V_hi = limbs 2..4
    std::vector<int64_t> h_vfixed_hi;
    int64_t total_fixed_hi = 0;
    double lo_abs_sum = 0;      // sum_s |V_lo,s| * 2^-F: bound of the low limbs' contribution to any joint sum
    // sequence order of the bit rows: position p of a row = sequence seq_perm[p]; positions ascend in weight, so sequences of equal weight
    // (a weight CLASS) are contiguous.  digits / dig_a / dig_b are indexed by position.
    std::vector<int32_t> h_seq_perm;   // [Npad], -1 in the padding
    DevBuf seq_perm;
    void drop() { have_weights = false; }
    void mark_set() { have_weights = true; }
};

// The approximate-GEMM form of the weights (ldw_apx.hip): V_p ~ a_p * b_p * 2^e(macro step of p), one int8 MFMA pass with both operands masked
// by a digit; exact joint sums of the listed units by class-wise popcounts.  Written by prepare_apx_weights alone (from ldw_set_weights), so it
// describes the LAST weights: readers ask gate(have_weights).
struct ApxWeights {
    bool apx_ok = false;               // the weights allow the approximate path (precision and class structure)
    bool apx_fine = false;             // block exponents per MFMA k-step (32 positions) instead of per macro step (128): weights with a large dynamic range
    std::string apx_gate = "weights not set";   // "ok" or the gate that keeps the path off (ldw_path_report)
    DevBuf dig_a, dig_b;               // uint8 [Npad]
    DevBuf apx_shift;                  // int32 [2 KW]: right shift of the accumulators before MFMA k-step k (32 positions)
    int apx_e_last = 0;                // accumulators end in units of 2^apx_e_last (fixed-point units of V)
    int apx_transitions = 0;           // k-steps with a shift: each loses < 1 unit (of ITS exponent) of a joint sum
    double apx_lost_units = 0;         // what that adds up to in units of 2^apx_e_last (< 2: the exponents ascend)
    double apx_delta = 0;              // max_p |V'_p - V_p| / V_p
    std::vector<int64_t> h_vapx;       // [Npad] by SEQUENCE: V'_s = a b 2^e (exact integer)
    DevBuf pop_segs, pop_wbeg;         // popcount segments (PopSeg, ldw_pairs.h) and first segment of every 32-bit word (+1)
    DevBuf pop_vpos;                   // r05: int64 [Npad] fixed-point weight by POSITION (k_pair_sums_bits: weightings with many classes)
    int n_pop_segs = 0, n_classes = 0;
    const char *gate(bool have_weights) const { return have_weights ? apx_gate.c_str() : "weights not set"; }
};

// Per-SNP meta data.  Written by ldw_set_snp_meta, or by ldw_set_positions (positions and g alone: pos_only); dropped by a new alignment shape.
struct SnpMeta {
    bool have_meta = false;
    bool pos_only = false;       // ldw_set_positions: L, POS and g stand for a job whose alignment is not here (no states, weights, r, uqe or paint)
    double g = 0;
    DevBuf r, uqe, POS, paint;   // double[L], uint8[L][5], int32[L], int32[L]
    std::vector<double> h_r;
    std::vector<int32_t> h_POS, h_paint;
    int32_t paint_min = 0, paint_max = 0;
    double r_min = 0;            // smallest r of the alignment (ldw_set_snp_meta)
    bool pos_sorted = true;      // POS ascends over the whole alignment (the reference's parser emits it so; any order is accepted)
    bool pos_strict = true;      // ... strictly: the SNP index is the rank among the distinct positions (no slot array needed)
    // The ascending order of the positions (ldw::pos_order builds it on first use; set_positions drops it), int32[L] each on the device:
    struct PosOrder {
        DevBuf order;            // the SNP of every sorted entry, SNPs of one position in index order  (not built when pos_sorted: it is the identity)
        DevBuf srt;              // the sorted positions                                               (not built when pos_sorted: POS itself)
        DevBuf slot;             // per SNP the rank of its position among the distinct positions      (not built when pos_strict: the SNP index)
        int64_t n_slots = 0;     // number of distinct positions; 0 = not built for the current positions
    } pos_ord;
    void drop() { have_meta = pos_only = false; }
    void mark_set(bool positions_only) { have_meta = true, pos_only = positions_only; }
    // the host copy of new positions and what is known of their order; the order built from the old ones (ldw::pos_order) is dropped
    void set_positions(const int32_t *POS_, int64_t L) {
        h_POS.assign(POS_, POS_ + L);
        pos_sorted = true;
        for (int64_t i = 1; i < L && pos_sorted; ++i) pos_sorted = POS_[i] >= POS_[i - 1];
        pos_strict = pos_sorted;
        for (int64_t i = 1; i < L && pos_strict; ++i) pos_strict = POS_[i] > POS_[i - 1];
        pos_ord.n_slots = 0;
    }
};

// What a pass learnt to size the short-range table with.  Written by ldw_mi_all_pairs; forgotten with the positions (new SNP meta, ldw_set_positions).
struct SrSizing {
    double sr_total_dist = -1;   // number of SNP pairs within sr_total_dist on the circle (sizes the short-range table once; reset with the meta data)
    int64_t sr_total = -1;
    uint64_t sr_share_key = 0;   // r05: the last SHARE of the block list a pass was sized for (hash of blocks + sr_dist) and its exact short-range row count
    int64_t sr_share_rows = -1;
    void learn_share(uint64_t key, int64_t n_rows) { sr_share_key = key, sr_share_rows = n_rows; }
    void forget() { sr_total = sr_share_rows = -1, sr_total_dist = -1; }   // (sr_share_key stays: it is read only beside sr_share_rows >= 0)
};

// The row map: which (SNP, state) pairs get an indicator row, built lazily by ensure_rows from alignment + weights + meta.  Invalid once any
// of the three is replaced; slot_pfix_hi is built on demand for the current map (ensure_hi_marginals); prep_block fills order_cache.
struct OrderCache { std::vector<int32_t> idx, order; };
struct RowMap {
    bool rows_ready = false;
    int64_t R = 0;               // number of indicator rows over all SNPs
    DevBuf Mbits;                // uint64 [R + TILE][KW]: bit s set where sequence s carries the row's state
    DevBuf row0;                 // int32 [L+1]: first row of each SNP
    DevBuf slot_meta;            // uint32 [L]: nrows (3 bits) | uq-by-slot (5 bits <<3) | slot states (5 x 3 bits << 8)
    DevBuf slot_pfix;            // int64 [L][5]: fixed-point marginal of the state in each slot
    DevBuf slot_pfix_hi;         // the same for the high-limb weights V_hi (nlimbs == 5), built on demand
    bool hi_ready = false;
    DevBuf slot_papx;            // int64 [L][5] by slot: floor(marginal of V' / 2^apx_e_last)
    DevBuf counts;               // int32 [L][5] per-SNP state counts
    DevBuf pfix_state;           // int64 [L][5]: fixed-point marginal of each state (histogram engine)
    // Per-SNP bound behind the pruning of the wider tables (k_snp_sup): snp_sup[a * 4 + 2 * m + (k - 2)] = the largest MI SNP a (2 or
    // 3 states, all flagged, r = its number of states) can reach with ANY partner of k = 2 or 3 flagged states and r = k, in the
    // intended (m = 0) and the reference (m = 1: RXY at its floor r_min^2 / 4) reading of RXY; +inf for other SNPs.
    DevBuf snp_sup;
    std::vector<int32_t> h_row0;
    std::vector<uint32_t> h_slot_meta;
    std::vector<int32_t> h_counts;
    std::vector<int64_t> h_minor_w;   // [L]: fixed-point weight of slot 0 of a biallelic r = 2 SNP with one row (else INT64_MAX)
    std::vector<int32_t> h_span_bad;  // [L + 1] prefix count of the SNPs a span cannot hold: no indicator row, or 1-2 rows with an unflagged slot (ensure_rows)
    std::mutex order_mtx;             // guards order_cache (prep_block runs on the helper thread and, for the cold-start probes, on the calling thread at once)
    std::vector<std::unique_ptr<OrderCache>> order_cache;   // per SNP list: its one-row SNPs in ascending order of the minor state's weight
    void invalidate() { rows_ready = false; }
    void rebuilt() { rows_ready = true, hi_ready = false, order_cache.clear(); }   // (hi_ready: made when a block first takes the mixed-precision path)
};

// What the passes learnt about the current problem in order to speculate: the bucket guesses of the long-range gather, and the threshold
// tables of the biallelic pairs, which depend on the weights alone.  Written by the block loop (ldw_mi_items.inc, ldw_mi_block.inc).
struct Speculation {
    bool spec_seen[2] = {false, false};  // a block of this kind (off-diagonal, diagonal) has set its own guess
    bool spec_probed[2] = {false, false};   // the kind's current guess came from a cold-start probe of the kind itself
    int spec_hist[2][6] = {{0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};   // the last true buckets per kind (adaptive margin of the guess)
    int spec_hist_n[2] = {0, 0};
    bool spec_small[2] = {false, false};   // the kind's blocks keep few rows (< 5000): noisier thresholds, wider margins
    int spec_B_next[2] = {-1, -1};       // bucket guess for the speculative long-range gather: [off-diagonal, diagonal]
    bool maybe_off = false;              // the maybe list overflowed in this pass: off until ldw_reset_speculation (new weights do NOT switch it on again)
    DevBuf tab11[2];                   // threshold tables of the biallelic pairs (k_build_tab11), int2 [nb][nb]: [off-diagonal, diagonal] blocks
    double tab11_lo[2] = {0, 0};       // MI level each was built for (0: none)
    int tab11_cur[2] = {0, 0};         // r04: each kind's buffer holds a RING of 4 tables; this one is current (a rebuild takes the next: items in flight keep theirs)
    float tab11_c = 0;
    int tab11_nb = 0;
    // bucket guesses of an earlier alignment / weighting say nothing about a new row map
    void forget_guesses() {
        spec_B_next[0] = spec_B_next[1] = -1;
        spec_seen[0] = spec_seen[1] = spec_probed[0] = spec_probed[1] = false;
        spec_hist_n[0] = spec_hist_n[1] = 0;
    }
    void drop_tables() { tab11_lo[0] = tab11_lo[1] = 0; }   // the threshold tables belong to the old weights
    void reset() { forget_guesses(), drop_tables(), maybe_off = false; }   // ldw_reset_speculation
};

// The device-resident link tables and the per-block records of the pass that made them.  Written by a pass (ldw_links_begin ..
// ldw_links_end), ldw_links_import, ldw_links_load and ldw_mi_all_pairs_multi's adoption; emptied by ldw_set_positions.  The kept links
// (KeptLinks, a sibling member of the context) index these tables: whatever replaces a table goes through replaced().
struct LinkTables {
    DevBuf sr_a, sr_b, sr_mi, lr_a, lr_b, lr_mi;
    int64_t n_sr = 0, n_lr = 0;
    int64_t blk_capacity = 0, blk_cursor = 0;  // ldw_links_begin / ldw_mi_block_links / ldw_links_end
    std::vector<BlockStat> stats;
    std::vector<int32_t> multi_owner;    // r05: ctx[0] of ldw_mi_all_pairs_multi(.., LDW_MI_SR_ROWS_STAY): the deal (owner of every block); empty otherwise
    void drop_deal() { multi_owner.clear(); }   // a deal describes the tables of the multi-context pass that made it only
    void new_pass() { n_sr = n_lr = 0, stats.clear(), drop_deal(); }   // ldw_links_begin (the kept links go when ldw_sr_pvalues counts anew)
    // whatever was derived from the old table is stale: the kept links, the per-block records of the pass that made it (ldw_block_stats
    // answers LDW_ERR_ARG until the next pass) and the deal of an in-process pass whose shares these rows replace
    void replaced(KeptLinks &kept) { kept.invalidate(), stats.clear(), drop_deal(); }
    void clear(KeptLinks &kept) { n_sr = n_lr = 0, replaced(kept); }
};

// What the reports read (ldw_ctx_counters*, ldw_*_report, ldw_gemm_stats): all count since the context was created; nothing drops them.
struct PassCounters {
    int64_t apx_blocks = 0, apx_units_listed = 0, apx_pairs_listed = 0, probe_blocks = 0, generic_blocks = 0;
    // launches by form (ldw_pair_form_report): [0] k_pair_sums_bits within the default 64 KB of LDS, [1] k_pair_sums_bits with the 160-KB attribute,
    // [2] k_pair_sums with its segment tables in LDS, [3] k_pair_sums with them in global memory, [4] k_fill_rows_bits in its global-memory form
    int64_t form_launches[5] = {0, 0, 0, 0, 0};
    // launches of the class-wise pair sums by kernel (ldw_pair_kernel_report): [0] a quarter-wave per pair (k_pair_sums_q), [1] a wave per pair (k_pair_sums)
    int64_t pair_kernel_launches[2] = {0, 0};
    int64_t apx_waves_skipped = 0, apx_waves_total = 0;
    int64_t tab11_builds = 0;
    int64_t slot_grown = 0;              // reallocations of a slot buffer where it is used (launch_block_apx; ldw_slot_report out[0])
    int64_t maybe_entries = 0;           // entries handed to the maybe list since the context was created (ldw_overflow_report out[3])
    int64_t pair_list_overflows = 0, maybe_overflows = 0;   // blocks / segments redone because a pair list / the maybe list overflowed (ldw_overflow_report)
    int64_t span_items = 0, span_blocks = 0, span_fallbacks = 0;   // spans run, reference blocks they covered, segments redone non-speculatively
    std::atomic<int64_t> sorted_blocks{0};   // (prep_block runs on the helper thread and, for the cold-start probes, on the calling thread at once)
    int64_t spec_misses = 0, blocks_run = 0, screen_violations = 0, mixed_blocks = 0;
    double gemm_stat[6] = {0, 0, 0, 0, 0, 0};   // ldw_gemm_stats: launches and executed int8 ops of the block-wide GEMMs
};

// The run-time switches (ldw_set_*); a context keeps them for life.
struct Knobs {
    int engine = LDW_ENGINE_MFMA;
    int path_mode = 0;                 // ldw_set_path: 0 auto, 1 mixed/plain path, 2 force the approximate path
    int select_mode = 0;               // ldw_set_select: 0 auto (sort-free selection where it applies), 1 always the two radix sorts
    int mixed = 1;                     // 1: high-limb GEMM + gathered low-limb GEMM for the listed units in speculative blocks
    // Tile pruning (docs/HISTORY.md 5.1d): in blocks without a short-range pair the one-row SNPs are ordered by the weight of their minor
    // state, so that a wave tile of the approximate GEMM spans few bins of the threshold table; a tile whose whole bin rectangle is
    // unconditionally below the level (no joint count can lift such a pair to it) is flagged clean without being computed.
    bool prune = true;                 // LDW_NO_PRUNE switches ordering and skipping off (A/B measurements)
    // Spans (r04, docs/HISTORY.md 6b): consecutive long-range-only blocks of one block row run as ONE launch sequence over their concatenated to side
    bool span_on = true;               // ldw_set_span / LDW_NO_SPAN
    int span_max = 8;                  // most reference blocks per span (LDW_SPAN_MAX env, <= ldw::LDW_SPAN_MAX)
    bool overlap = true;               // GEMM of block b+1 on its own stream beside the epilogue/selection of block b
    int screen = 1;                    // fp32 screen in front of the fp64 MI evaluation (0 off, 1 on, 2 verify)
};

// LDW_HOST_TIMING: the host's wall clock around the steps of the larger entry points, printed to stderr
inline bool host_timing() {
    static const bool on = getenv("LDW_HOST_TIMING") != nullptr;
    return on;
}
struct HostClock {
    using Point = std::chrono::steady_clock::time_point;
    static Point now() { return std::chrono::steady_clock::now(); }
    static double ms(Point a, Point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
    static double us(Point a, Point b) { return std::chrono::duration<double, std::micro>(b - a).count(); }
};
}  // namespace ldw

// Every GPU resource below is an owning member (ldw_own.h): `delete` gives all of it back, in reverse order of declaration, so the streams
// come first and go last.  ldw_ctx_destroy drains them before it deletes.
struct ldw_ctx {
    int device = 0;
    int n_cu = 0;                    // compute units of the device (hipDeviceProp_t::multiProcessorCount): sizes the approximate GEMM's list launch
    ldw::Stream stream;              // the main stream: the library's own, or the caller's (ldw_ctx_set_stream: adopted, never destroyed here)
    ldw::Stream copy_stream, gemm_stream;   // pipelined block staging (ensure_streams): host prep of block i+1 overlaps the GPU work of block i
    ldw::Stream lr_st;               // the streaming lr_links.tsv writer's (ensure_streams)
    bool streams_ready = false;      // ensure_streams has made everything it makes
    ldw::Event ev[6];
    double last_ms[4] = {0, 0, 0, 0};

    // ---- alignment ----
    int64_t L = 0, N = 0, Npad = 0;  // Npad: N rounded up to a multiple of KSTEP (128)
    int64_t KW = 0;                  // 64-bit words per bit row = Npad / 64
    ldw::DevBuf states;              // uint8 [L][N]
    ldw::DevBuf chars;               // raw alignment characters [cN][cL] kept by ldw_alignment_scan
    int64_t cN = 0, cL = 0;
    void *fasta = nullptr;           // scan state of the native FASTA feeder (ldw_fasta.hip: FastaScan), made by ldw_fasta_scan
    void *out = nullptr;             // staging of the alignment writer (ldw_out.hip: OutState), made by ldw_write_alignment
    void *tsv = nullptr;             // the link-table reader (ldw_links_read.hip: TsvState), made by ldw_tsv_read
    void *grep = nullptr;            // the search of annotated link files (ldw_links_grep.hip: GrepState), made by ldw_links_grep

    // ---- the sub-states (above), in the order of the chain: what the problem is, what is derived from it, what the passes leave ----
    ldw::Weights wts;
    ldw::ApxWeights apx;
    ldw::SnpMeta meta;
    ldw::SrSizing sizing;
    ldw::RowMap rows;
    ldw::Speculation spec;
    ldw::LinkTables links;
    ldw::KeptLinks kept;         // the kept links, their ARACNE pool and flags
    ldw::SrModel srm;            // the short-range model's buffers and the geometry of the last quantile call
    ldw::PassCounters cnt;
    ldw::Knobs knobs;
    // The chain, stated once (DESIGN.md 27 has it as a table).  A new alignment shape (set_dims) drops the weights and the meta data ...
    void new_shape() { wts.drop(), meta.drop(), rows.invalidate(); }
    // ... positions without an alignment (ldw_set_positions) are that, and the tables index the old SNPs;
    void positions_only() { new_shape(), links.clear(kept), sizing.forget(); }
    // new weights: the row map holds the old marginals, the threshold tables the old weights' levels;
    void new_weights() { wts.mark_set(), rows.invalidate(), spec.drop_tables(); }
    // new SNP meta data: the row map holds the old flags and r, the sizing counted the old positions (their order went in set_positions);
    void new_meta() { meta.mark_set(false), rows.invalidate(), sizing.forget(); }   // (pos_only is false already: the setter needs an alignment)
    // a rebuilt row map (ensure_rows): nothing learnt about the old one holds.
    void rows_rebuilt() { rows.rebuilt(), spec.forget_guesses(); }

    // ---- per-slot pipeline buffers of the approximate path (ldw_slots.h) ----
    bool pair_bits_attr = false;       // the > 64 KB dynamic-LDS attribute of k_pair_sums_bits has been set (this context's device)
    ldw::DevBuf panel[LDW_NSLOT][2];           // [slot][from, to]: packed bit panels of a block's row lists, [KW/2][Rpad][2] u64
    ldw::DevBuf Gapx[LDW_NSLOT];               // int32 [RTpad][RFpad] approximate joint sums, one per pipeline slot
    ldw::DevBuf pair_sums;             // exact joint sums of the listed pairs (16 per pair)
    ldw::DevBuf pairs[LDW_NSLOT];              // per pipeline slot: pair lists of the approximate screen (counters + PAIR_PATHS x PAIR_SHARDS lists)
    ldw::DevBuf apx_bins[LDW_NSLOT], apx_clean[LDW_NSLOT];    // per slot: threshold-table bin of every row of the two row lists; clean-region flags of the GEMM epilogue
    ldw::DevBuf apx_mini[LDW_NSLOT];           // per slot: the 32-byte per-SNP extracts k_screen_maybe reads (MiniCol [nt], MiniRow [64 * from-tiles])
    ldw::DevBuf apx_units[LDW_NSLOT], apx_packs[LDW_NSLOT];   // per slot: per-(tile, class) unit lists + counters; per-block SNP constants
    ldw::DevBuf apx_skip;              // uint64: wave tiles the GEMM skipped since the counter was last read
    double apx_ops_per_wave = 0;       // executed-operation accounting of the skipped tiles (ldw_gemm_stats)
    bool early_sr = false;             // this pass assigns an item's short-range rows when the item is SUBMITTED (submit order = block order), not in its second phase
    ldw::DevBuf glo;             // int32: low-limb joint sums of the listed units (gathered GEMM)
    ldw::DevBuf lo_rows;         // int32 row lists of the gathered GEMM's workgroups
    ldw::DevBuf packs;           // per-block SNP constants in epilogue order (ColMeta / RowPack arrays, k_build_packs)
    // ---- CDS variation / paint (ldw_cds.hip) ----
    ldw::DevBuf cds_keep;        // uint32 [cds_L] positions in ascending order, int32 [cds_L] their SNP index: left by ldw_cds_variation for ldw_cds_paint
    ldw::DevBuf cds_work;        // per-call working memory of both
    int64_t cds_L = 0;           // SNPs of the last ldw_cds_variation (0: none yet)
    ldw::DevBuf annot_keep;      // int32 [2][annot_n] annotation row of every link end: left by ldw_annot_map for ldw_annot_links
    ldw::DevBuf annot_work;      // per-call working memory of ldw_annot_map / ldw_annot_links / ldw_annot_snps
    int64_t annot_n = -1, annot_rows = 0;   // links and annotation rows of the last ldw_annot_map (-1: none yet)

    // ---- per-block workspaces ----
    ldw::DevBuf G, G2, G3;       // int64 [RTpad][RFpad] fixed-point joint sums, one per pipeline slot (gx())
    ldw::DevBuf MIblk;           // double [nf*nt]
    ldw::DevBuf rowlist_f, rowlist_t, idx_f, idx_t, lrow_f, lrow_t, perm_f, perm_t;
    ldw::DevBuf epi_rest;        // plain path's epilogue: counter (64-B slot) + list of the units k_mi_epilogue_fast left to k_mi_epilogue_rest
    ldw::DevBuf scr_units;       // uint32 count (64-B slot) + list of the block's units the fp32 screen wants evaluated exactly
    ldw::DevBuf hist[LDW_NSLOT], cand_key[LDW_NSLOT], cand_val[LDW_NSLOT];   // per pipeline slot: histogram of the lr candidates, candidate list
    ldw::DevBuf colcnt, cand_key2, cand_val2, scratch, small;
    ldw::DevBuf miss_key, miss_val;   // candidate list of a span's segment that is redone on its own (the slot's lists hold its neighbours')
    std::vector<uint8_t> ev_valid;    // per block of the pass: its stage events were recorded (the segments of a span share the first one's)
    ldw::DevBuf sel_bitmap, sel_chunks, sel_prefix;   // fast selection (k_sel_thresh): bitmap, chunk and super-chunk (sel_prefix) counters, all-zero between blocks

    // ---- the link-table writers (ldw_tsv.cpp) ----
    void *lr_stream = nullptr;   // r05: lr_links.tsv appended while the pass runs (ldw_tsv.cpp: LrStream), if ldw_lr_stream_begin opened one
    // its device-side resources (with lr_st), made once with the context's other streams (hipStreamCreate is a 12-ms call: not inside a job's pass)
    ldw::Event lr_ev[64];
    ldw::PinnedBuf lr_counts;    // int64 [64]
    ldw::PinnedBuf lr_pin;       // pinned staging of a batch of rows (a, b, MI); grows on demand
    void *tsv_async = nullptr;   // r04: the asynchronous link-table writer, if one is running (ldw_tsv.cpp: TsvAsync)
    ldw::PinnedBuf pin_fetch;    // r04: pinned host arena the tsv writer fetches a link table into (see ldw_write_links_tsv)
    int64_t decay_stat[4] = {0, 0, 0, 0};            // ldw_decay_report: patches, route-B patches, pairs outside their patch's bound and blocks of the last ldw_mi_profile
    int64_t snpsum_stat[5] = {0, 0, 0, 0, 0};        // ldw_snp_summary_report: patches, general-route patches, pairs off their patch's class, values q refused and blocks of the last ldw_mi_snp_summary
    int64_t scoresel_stat[3] = {0, 0, 0};            // ldw_score_select_report: patches visited, NaN scores and blocks of the last ldw_mi_score_scan or ldw_mi_score_links
    int64_t segmap_stat[5] = {0, 0, 0, 0, 0};        // ldw_segment_map_report: patches visited, patches on route 2, values q refused, NaN values and blocks of the last ldw_mi_segment_map or ldw_mi_segment_best
    double ham_stat[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // ldw_hamming_stats: columns, padded K, stage times and algorithmic bytes of the last ldw_hamming_weights
    ldw::DevBuf plot_work, plot_cols;   // the plots (ldw_plot.hip): key image + rasters + partials; device copy of a chunk of host columns

    // ---- pipelined block staging ----
    ldw::Event ev_gemm[LDW_NSLOT];
    ldw::PinnedBuf pin[LDW_NSLOT + 1];   // pinned host staging, one packed buffer per slot (+ 1: a span segment that is redone on its own)
    ldw::DevBuf dstage[LDW_NSLOT + 1];               // device image of the packed buffer
    ldw::Event ev_up[LDW_NSLOT], ev_done[LDW_NSLOT];
    bool done_recorded[LDW_NSLOT] = {};
    bool up_recorded[LDW_NSLOT] = {};    // ev_up[slot] has been recorded at least once
    ldw::PinnedBuf pin_pick[LDW_NSLOT];   // pinned landing zone of the per-block PickOut, one per slot
    ldw::Event ev_pick[LDW_NSLOT];
    ldw::Event ev_probe[2];           // one per cold-start probe of a pass: the calling thread waits for the probe it needs, not for the stream
    ldw::PinnedBuf pin_lrc;              // pinned copy of the running long-range row count
    ldw::Event ev_lrc;
    bool lrc_recorded = false;
    std::vector<ldw::Event> ev_pool;     // 4 timing events per block
    std::vector<ldw::BlockTrace> trace;
    // ldw_ctx_reserve (r04): what a job's FIRST pass otherwise pays inside its timed loop — two hipStreamCreate (12 ms each on this box), the
    // pinned staging buffers (hipHostMalloc: 0.2 ms per MB), the lazy load of the code objects of the pass's kernels — done by a side thread
    // while the caller uploads the alignment and runs the Hamming GEMM.  Joined by every entry point that uses what it prepares.
    std::thread prep_thread, prep_thread2;   // started by ldw_ctx_create (streams, code objects) / ldw_ctx_reserve (staging buffers)
    int prep_rc = 0, prep_rc2 = 0;
    std::string prep_err, prep_err2;
};

namespace ldw {
// launchers implemented in the .hip files (all asynchronous on ctx->stream)
int ensure_rows(ldw_ctx *ctx);
int set_dims(ldw_ctx *ctx, int64_t L, int64_t N);   // ldw_api.hip: the shape of the resident alignment; reserves states [L][Npad]
// G[t][f] = sum_k [row t has bit k][row f has bit k] * sum_j digits[j][k] 256^j over the bit matrix Mbits[rows][KW words]
int launch_gemm_bits(ldw_ctx *ctx, const uint64_t *Mbits, int64_t KW, const int32_t *rowlist_t, int RTpad, const int32_t *rowlist_f,
                     int RFpad, int64_t *G, int nlimbs, const int8_t *digits, int lower_only, hipStream_t stream = nullptr, int by0 = 0,
                     int by1 = -1,    // by0..by1: strip of 128-row to-side tiles to compute (default: all)
                     const uint8_t *tile_mask = nullptr,    // [RTpad / 128][RFpad / 64]: 0 = skip the tile (default: all tiles)
                     const uint32_t *tile_list = nullptr, int n_tile_list = 0);   // r06: the same tiles as a list (by << 16 | bx): a 1-D grid of exactly those
// the same exact sums (all limbs) by class-wise popcounts over the bit rows (ldw_hist.hip, LDW_ENGINE_HIST)
int launch_cooc_popc(ldw_ctx *ctx, const int32_t *rowlist_t, int RTpad, const int32_t *rowlist_f, int RFpad, int64_t *G, int lower_only,
                     hipStream_t stream = nullptr);
int fill_rows_bits(ldw_ctx *ctx, const int32_t *d_rowinfo, int64_t R);
int prepare_apx_weights(ldw_ctx *ctx);   // ldw_apx.hip: dual digits, exponents and the popcount segment tables (ldw_pairs.h) from h_vfixed / h_seq_perm
int check_gpu(ldw_ctx *ctx);
inline bool have_alignment(const ldw_ctx *ctx) { return ctx->L > 0 && !ctx->meta.pos_only; }   // (ldw_set_positions sets L without one)
int ensure_hi_marginals(ldw_ctx *ctx);   // slot_pfix_hi on demand (mixed-precision path)
// ldw_mi.hip: run_block_mi without link tables, as ldw_mi_block runs it: the dense MI of one block into ctx->MIblk [nf * nt] column-major; the block's index
// lists stay in ctx->idx_f / idx_t, its stage events are ctx->ev[0..2] (ldw_decay.hip)
int block_mi_dense(ldw_ctx *ctx, const int32_t *from_idx, int64_t nf, const int32_t *to_idx, int64_t nt, int quirk);
// ldw_decay.hip: what ldw_mi_profile, ldw_mi_snp_summary and the two entries of ldw_scoresel.hip share.  pair_blocks_check: the requirements of both entries (a GPU, the arguments, the quirk mode, the
// resident alignment, weights and meta data, then own_check() for the caller's own arguments, then every block diagonal or disjoint), refused under the caller's name.  pair_blocks_walk: per block the dense MI
// (block_mi_dense), consumer(nf, nt, diag) launched behind it on the context's stream, the synchronisation, and the event times and pair count added to W.
struct PairBlockWalk {
    double ms_mi = 0, ms_consumer = 0;   // the blocks' GEMM + epilogue; the consumer's kernels
    int64_t npairs = 0;
};
int pair_blocks_check(ldw_ctx *ctx, const char *who, const int32_t *blocks, int64_t nblocks, int quirk_mode, bool outputs_ok, const std::function<int()> &own_check);
int pair_blocks_walk(ldw_ctx *ctx, const int32_t *blocks, int64_t nblocks, int quirk_mode, PairBlockWalk &W, const std::function<int(int64_t, int64_t, bool)> &consumer);
void lr_stream_push(ldw_ctx *ctx, hipStream_t s, const int64_t *d_lr_count, int64_t blocks_done);   // ldw_tsv.cpp: no-ops without an open stream
void lr_stream_drain(ldw_ctx *ctx);
int join_prepare(ldw_ctx *ctx);      // waits for the side thread of ldw_ctx_reserve (no-op without one); its error, if any, becomes the caller's
int reserve_slot_buffers(ldw_ctx *ctx, int64_t Npad, int64_t blk, int64_t nseg);   // ldw_mi.hip: per-slot device buffers from the block geometry
int ensure_streams(ldw_ctx *ctx);    // the copy / GEMM streams, per-slot events and pinned pick records of the all-pairs loop (once per context)
void warm_mi();                      // lazy code-object loads of the translation units whose kernels a pass launches (hipFuncGetAttributes)
void warm_apx();
void warm_pairs();
void warm_gemm_bits();
void ctx_count(int d);               // ldw_alloc.cpp: live contexts of the process (the last one to go trims the device free list to its idle cap)
struct DrainedScope { DrainedScope(); ~DrainedScope(); };   // releases inside: the caller has drained every stream that could touch the blocks
int launch_state_counts(ldw_ctx *ctx);   // ldw_api.hip: per-SNP state counts into ctx->rows.counts on the context's stream (no copy, no synchronisation)
size_t device_pool_trim();          // ldw_alloc.cpp: give the released device blocks kept for re-use back to the runtime (ldw_host_trim); bytes
void warm_srp();
// ldw_srp.hip: ldw_sr_reduced_import with the kept links' meta words (clust_c | first << 8 | dup << 16) and srp values (both may be null)
int reduced_import_full(ldw_ctx *ctx, int64_t n_red, const int32_t *a, const int32_t *b, const double *MI, const uint32_t *meta, const double *srp, int64_t n_pool,
                        const int32_t *pool_a, const int32_t *pool_b, const double *pool_MI);
void warm_post();
// ldw_post.hip: the graph node of every SNP for consumers that work on positions (LD map, ARACNE): *slot = null and *n_nodes = L when POS
// ascends strictly, else the device array ctx->pos_ord.slot (SNPs sharing a position share a node) and the number of distinct positions
int pos_slots(ldw_ctx *ctx, const int32_t **slot, int64_t *n_nodes);
// a sub-state of the context (ctx->fasta, out, tsv, grep: a struct of owning members behind a void *) goes, once the main stream is idle
template <class T> void release_state(ldw_ctx *ctx, void *&state) {
    if (!state) return;
    (void)hipStreamSynchronize(ctx->stream);
    delete static_cast<T *>(state);
    state = nullptr;
}
// n items of host memory into a device buffer grown to hold them, queued on the main stream (the source stays valid until the stream has passed the copy)
template <class T> int upload(ldw_ctx *ctx, DevBuf &b, const T *src, size_t n) {
    if (int rc = b.reserve(std::max<size_t>(n, 1) * sizeof(T))) return rc;
    if (n) LDW_HIP(hipMemcpyAsync(b.p, src, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return LDW_OK;
}
// The frame of an entry point that works in buffers of its own (a struct of DevBufs) rather than the context's: run(bufs), then the buffers go.
// This context's stream alone touched the blocks: once it is idle they go without a device-wide synchronisation each (other contexts of the
// device may be in the middle of a pass).  A failed launch has queued nothing behind it; a stream that does not drain leaves them to the destructors.
template <class Bufs, class Run> int scoped_call(ldw_ctx *ctx, Run run) {
    if (int rc = check_gpu(ctx)) return rc;
    Bufs bufs;
    const int rc = run(bufs);
    if (hipStreamSynchronize(ctx->stream) == hipSuccess) {
        DrainedScope quiet;
        bufs = Bufs();
    }
    return rc;
}
// The events a chunked call records on its stream, one after the other, and the time between them once the stream has drained
struct Laps {
    std::vector<Event> ev;
    int mark(hipStream_t s) {   // one more event, recorded
        ev.emplace_back();
        LDW_HIP(ev.back().ensure());
        LDW_HIP(hipEventRecord(ev.back(), s));
        return LDW_OK;
    }
    // ms[k % period] += the time from event k to event k + 1.  group > 0: the events come in groups of that many, k counts within its group, and
    // the time from the last event of a group to the first of the next is nobody's
    int sums(int period, double *ms, int group = 0) const {
        for (size_t k = 0; k + 1 < ev.size(); ++k) {
            const size_t in = group ? k % (size_t)group : k;
            float x = 0;
            if (group && in + 1 == (size_t)group) continue;
            LDW_HIP(hipEventElapsedTime(&x, ev[k], ev[k + 1]));
            ms[in % (size_t)period] += x;
        }
        return LDW_OK;
    }
};
void out_release(ldw_ctx *ctx);      // ldw_out.hip: the alignment writer's staging (ldw_ctx_destroy)
int64_t out_trim(ldw_ctx *ctx);      // ... its pinned buffers and device image only (ldw_host_trim); bytes released
}  // namespace ldw
