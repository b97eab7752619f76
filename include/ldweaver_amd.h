/*
 * ldweaver_amd.h — C ABI of the MI355X-native all-pairs weighted-MI engine: the integration surface.
 *
 * This is the drop-in boundary for the ONE hot path of Sudaraka88/LDWeaver:
 *   perform_MI_computation()            R/computePairwiseMI.R:46-145
 *   estimate_Hamming_distance_weights() R/performPopulationStuctureCorrection.R:20-81
 *   .ACGTN2num()                        src/ACGTN2num_parallel.cpp:10-43
 *   estimate_variation_in_CDS()         R/estimateCDSDiversity.R:27-210
 * and the native helpers they call through `.Call` (src/RcppExports.cpp:154-167).
 *
 * Every entry point is `extern "C"`, takes plain pointers and sizes (no R, Rcpp or
 * torch types), returns an int status (0 = LDW_OK) and leaves a thread-local
 * message retrievable with ldw_last_error().  The caller allocates every output
 * (variable-length link tables use a two-call size query).  The R-side binding a
 * maintainer would add is shown in INTEGRATION.md and kept as source in r_shim/.
 *
 * Diagnostics, test hooks and execution options that change no result are declared
 * in ldweaver_amd_debug.h.  A binding needs none of them.
 *
 * Conventions
 *   states  uint8 [L][N] row-major, values 0..4 = A,C,G,T,N: the dense equivalent of the five
 *           one-hot sparse matrices of `snp.dat` (R/extractSNPs.R:138-141), encoded by the rule of
 *           src/getACGTNsites.cpp:229-265.
 *   SNP indices in block descriptors are 1-based inclusive like make_blocks()
 *           (R/computePairwiseMI.R:147-165); index arrays are 0-based.
 *   MI blocks are column-major nf x nt doubles, element (a,b) at a + b*nf, exactly the R matrix
 *           `MI` of perform_MI_computation_ACGTN (R/computePairwiseMI.R:268).
 *   on_device != 0 means the named pointers are device pointers on the context's GPU; 0 means host memory.
 *
 * Streams and synchronisation
 *   A context's kernels and copies run on its stream (its own, or the caller's: ldw_ctx_set_stream) and on
 *   helper streams the context owns.  Host outputs are complete when a call returns.  Calls that read or
 *   write caller device memory synchronise before they return, except ldw_acgtn2num_dev and
 *   ldw_fast_hadamard(on_device != 0), which only queue their kernel on the context's stream (ldw_ctx_sync
 *   waits for it).  A context must not be used from two threads at once.
 *   The caller's stream may be of any kind: non-blocking or blocking (default flags), of any priority, torch's current
 *   stream or not.  Work the caller has queued on it in front of a call needs no wait: the call's kernels and copies are
 *   ordered behind it by the stream.  The helper streams (block staging, the block-wide GEMMs, the streaming tsv writer)
 *   and the side threads stay the context's own whatever its main stream is; the helper streams are ordered against the
 *   main stream by events, never through the null stream.  Several contexts may run on the same caller's stream: their
 *   work is serialised on it in the order of the calls, results do not change (also under ldw_mi_all_pairs_multi).
 *   A stream handed in is never destroyed by the library and works on after the context has gone.
 *   (tests/test_caller_stream_gpu.py pins all of this.)
 *
 * Device memory handed out
 *   Device views handed out by ldw_links_device_ptrs and ldw_sr_tail_extract(on_device = 1) stay valid only
 *   until ldw_ctx_destroy.  ldw_ctx_destroy waits for the context's own streams, not for the caller's: the
 *   caller must synchronise every stream that reads these views (a torch or RCCL stream, say) before it
 *   destroys the context.  The views of ldw_links_device_ptrs point into the context's own table and end
 *   earlier, at the next call that changes that table.
 */
#ifndef LDWEAVER_AMD_H
#define LDWEAVER_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LDW_OK 0
#define LDW_ERR_ARG 1      /* bad argument (shape, range, null pointer)            */
#define LDW_ERR_HIP 2      /* a HIP runtime call or kernel launch failed            */
#define LDW_ERR_STATE 3    /* call order violated (e.g. MI before weights are set)  */
#define LDW_ERR_NOGPU 4    /* no usable gfx950 device: there is NO CPU fallback     */
#define LDW_ERR_SIZE 5     /* caller buffer too small (see the size query)          */

/* quirk modes of the block kernel */
#define LDW_QUIRK_REFERENCE 0 /* reproduce Q1: RXY read by linear index of the nt x nf matrix (R/computePairwiseMI.R:261 + src/computeMI.cpp:19) */
#define LDW_QUIRK_INTENDED 1  /* RXY = 0.25*r_a*r_b */

typedef struct ldw_ctx ldw_ctx;

/* ---- library / context ------------------------------------------------------------------ */
int ldw_version(void);
const char *ldw_last_error(void);
/* number of visible HIP devices (0 when none); never initialises a context */
int ldw_device_count(void);

/* A context owns one GPU's device buffers, streams and link tables.  LDW_ERR_NOGPU without a gfx950 device.  Creating one also starts
 * a side thread that loads the pass's kernels; every entry point that needs them waits for it. */
int ldw_ctx_create(int device, ldw_ctx **out);
/* Finishes pending tsv writers, waits for the context's own streams and side threads, and releases everything it owns.  Device blocks
 * of 64 MB or more go to a process-wide free list for the next context (ldw_host_trim gives them back).  See "Device memory handed
 * out" above: streams the caller owns are not waited for.  NULL is accepted. */
int ldw_ctx_destroy(ldw_ctx *ctx);
/* Optional: sizes the per-block device buffers and pinned staging buffers of the all-pairs loop for an L x N alignment and blocks of
 * at most max_blk_sz SNPs, on a side thread of the context.  Call it right after the alignment upload.  The entry points that use
 * these buffers wait for the thread; without this call they are made on first use.  Results do not depend on it. */
int ldw_ctx_reserve(ldw_ctx *ctx, int64_t L, int64_t N, int64_t max_blk_sz);
/* run everything on an externally owned hipStream_t (e.g. torch's current stream); NULL = own stream.  The context's current main
 * stream and its helper streams are synchronised first, so everything the context has queued is done before the stream changes; the
 * helper streams stay the context's own and the side threads of ldw_ctx_create / ldw_ctx_reserve are not waited for (they touch no
 * stream).  The call is therefore allowed between any two calls on the context: right after ldw_ctx_create, between the stages of a
 * job, between ldw_links_begin and ldw_links_end, and while ldw_lr_stream_begin or ldw_write_links_tsv_begin is open — tables and
 * files are the same as without it.  Adopting a stream destroys the context's own main stream (one stream fewer in
 * ldw_resource_report), NULL makes one again; the stream handed in is never destroyed, and the same one may be given to several
 * contexts (see "Streams and synchronisation"). */
int ldw_ctx_set_stream(ldw_ctx *ctx, void *hip_stream);
/* waits for the work queued on the context's stream */
int ldw_ctx_sync(ldw_ctx *ctx);
/* Releases the host memory the library keeps between calls: the tsv writers' process-wide buffer pool, the context's pinned fetch
 * arena (ctx may be NULL: the pool only), and the pooled device blocks that released buffers and destroyed contexts left for the
 * next taker.  Call it between jobs, not between the calls of one job: giving large host regions back next to GPU work stalls the
 * process's next GPU call (docs/HISTORY.md 8).  bytes_out: bytes released (may be NULL). */
int ldw_host_trim(ldw_ctx *ctx, int64_t *bytes_out);

/* ---- (1) .ACGTN2num  — src/ACGTN2num_parallel.cpp:10-43, R/RcppExports.R:4-6 ------------ */
/* nv: 5 x L doubles, column-major, mutated IN PLACE (host memory, as R hands it over);
 * ref: L bytes = first character of each element of `cv`; ncores is accepted and ignored. */
int ldw_acgtn2num(ldw_ctx *ctx, double *nv, const char *ref, int64_t L, int ncores);
/* same on device-resident buffers (no copies); queued on the context's stream, not waited for */
int ldw_acgtn2num_dev(ldw_ctx *ctx, double *nv_dev, const char *ref_dev, int64_t L);

/* ---- (3) .fastHadamard — src/computeMI.cpp:11-21, R/RcppExports.R:8-10 ------------------- */
/* element-wise twin over the linear index c < n; MI updated in place.  on_device != 0: all pointers
 * are device pointers and the kernel is queued on the context's stream, not waited for. */
int ldw_fast_hadamard(ldw_ctx *ctx, double *MI, const double *den, const double *uq, const double *pxy,
                      const double *pxpy, const double *RXY, const double *pXrX, const double *pYrY,
                      int64_t n, int on_device);

/* ---- alignment residency ------------------------------------------------------------------ */
/* Upload (on_device == 0) or adopt a copy of (on_device != 0) the L x N state matrix.  Weights and SNP meta data set before are dropped. */
int ldw_set_alignment(ldw_ctx *ctx, const uint8_t *states, int64_t L, int64_t N, int on_device);
/* 5-state encoder of src/getACGTNsites.cpp:229-265 on the device: chars [N][L_total] (sequence-major,
 * as a FASTA holds them) -> states [n_pos][N] for the 1-based retained columns pos[n_pos]; the result
 * becomes the context's alignment.  Also returns the 5 x n_pos ACGTN_table (may be NULL). */
int ldw_encode_alignment(ldw_ctx *ctx, const char *chars, int64_t N, int64_t L_total, const int32_t *pos,
                         int64_t n_pos, int32_t *acgtn_table_out);
/* First half of `extractAlnParam` (src/getACGTNsites.cpp:47-90): upload the raw alignment chars [N][L_total]
 * (they stay resident: a following ldw_encode_alignment may pass chars = NULL) and count A/a, C/c, G/g, T/t and
 * "everything else" per column: allele_counts_out is 5 x L_total int32, column-major like `allele_counts`.
 * The SNP filter itself (:104-166) is O(L_total) host logic on these counts. */
int ldw_alignment_scan(ldw_ctx *ctx, const char *chars, int64_t N, int64_t L_total, int32_t *allele_counts_out);
/* ---- the native FASTA feeder: a FASTA file (plain or gzip, read with zlib) streamed into the device scan and encoder without the
 * whole N x L_total character matrix ever existing, on the host or on the device (src/getACGTNsites.cpp:13-291).  Records: a header
 * line starts with '>', the name is its first whitespace-delimited token ("" if none); other lines are sequence with trailing '\r' /
 * '\n' stripped, blank lines skipped, every other byte kept; lines before the first header are skipped.  Errors (LDW_ERR_ARG):
 * "File does not contain any sequences!" and "sequences are of different lengths" (an empty record counts as one of length 0).
 * Names come NUL-separated (each followed by '\0'); names may be NULL, names_bytes receives the size needed (LDW_ERR_SIZE if
 * names_cap is smaller).  chunk_rows / io_bytes 0: the defaults (rows of about 32 MiB, 4 MiB reads). */
/* host only, no context and no GPU: parse the whole file and return its shape and names — for callers sizing buffers, and CPU tests */
int ldw_fasta_probe(const char *path, int64_t io_bytes, int64_t *N, int64_t *L_total, char *names, int64_t names_cap,
                    int64_t *names_bytes);
/* pass 1: stream the file, accumulate per-column allele counts on the device; keep the 4-bit packed states resident if they fit in
 * keep_bytes (0: never, < 0: automatic — at most 8 GiB and a quarter of the free device memory).  A new scan discards the last one. */
int ldw_fasta_scan(ldw_ctx *ctx, const char *path, int64_t chunk_rows, int64_t io_bytes, int64_t keep_bytes, int64_t *N_out,
                   int64_t *L_total_out);
/* the scan's A/C/G/T/other counts: 5 x L_total int32, column-major like `allele_counts` (ldw_alignment_scan) */
int ldw_fasta_counts(ldw_ctx *ctx, int32_t *allele_counts_out);
/* the scan's sequence names, NUL-separated as in ldw_fasta_probe (names may be NULL: size query) */
int ldw_fasta_names(ldw_ctx *ctx, char *names, int64_t cap, int64_t *names_bytes);
/* pass 2: encode the 1-based retained columns pos[n_pos] into the context's alignment (states [n_pos][N]); from the packed copy if the
 * scan kept one (released here), else by reading the file again (LDW_ERR_STATE if its size, modification time, N or L_total changed);
 * LDW_ERR_STATE without a scan.  acgtn_table_out as in ldw_encode_alignment (may be NULL). */
int ldw_fasta_encode(ldw_ctx *ctx, const int32_t *pos, int64_t n_pos, int32_t *acgtn_table_out);
/* per-SNP state counts (5 x L, column-major like ACGTN_table) of the resident alignment */
int ldw_state_counts(ldw_ctx *ctx, int32_t *counts_out);
/* copy the resident states back: L x N, the layout ldw_set_alignment takes */
int ldw_get_alignment(ldw_ctx *ctx, uint8_t *states_out);

/* ---- (2) estimate_Hamming_distance_weights — R/performPopulationStuctureCorrection.R:20-81 */
/* hdw_out[j] = 1 / (#{i : L - shared[i][j] < thresh} + 1), thresh = as.integer(L*threshold) computed by
 * the caller.  shared_out (N x N int32, may be NULL) receives the exact shared-state counts. */
int ldw_hamming_weights(ldw_ctx *ctx, int32_t thresh, double *hdw_out, int32_t *shared_out);
/* Sharded form: the N x N comparison is symmetric, so only pairs (t, f), t <= f, are computed; this entry
 * point does the strip of 128-sequence row tiles [tile0, tile1) (tile1 <= ceil(N / 128) rounded to the padding) and
 * returns counts_out[j] = the strip's contribution to #{i : L - shared[i][j] < thresh} for EVERY j in 0..N-1.  The strips
 * of all ranks add up to the full count n_j (self included), hdw[j] = 1 / (n_j + 1): exact integers, so every rank
 * derives bit-identical weights after one all-reduce of N counts. */
int ldw_hamming_counts(ldw_ctx *ctx, int32_t thresh, int32_t tile0, int32_t tile1, int64_t *counts_out);
/* ldw_hamming_weights over several contexts of this process holding the same alignment: the symmetric comparison is cut into strips of
 * equal area, one per context (ldw_hamming_counts), and the integer neighbour counts are added on the host: hdw_out[N] is
 * bit-identical to ldw_hamming_weights on one context. */
int ldw_hamming_weights_multi(ldw_ctx **ctx, int n_ctx, int32_t thresh, double *hdw_out);

/* ---- MI set-up ------------------------------------------------------------------------------ */
/* Per-sequence weights hdw[N] (R/computePairwiseMI.R:77,89).  The engine uses v_s = fl(sqrt(hdw_s))^2
 * like the reference's sqrt-scaled one-hots, quantised to nlimbs*8-bit fixed point (nlimbs in 1..6,
 * 0 = default 5).  Needs the alignment. */
int ldw_set_weights(ldw_ctx *ctx, const double *hdw, int64_t N, int nlimbs);
/* r[L] (snp.dat$r), uqe[L][5] row-major 0/1 (snp.dat$uqe), POS[L] (snp.dat$POS: any order, like the reference; blocks whose positions
 * ascend take the fast paths, a block in another order runs the plain path), paint[L] (cds_var$paint), g genome length (snp.dat$g).
 * Needs the alignment.  Finishes a pending asynchronous tsv table of the context first. */
int ldw_set_snp_meta(ldw_ctx *ctx, const double *r, const uint8_t *uqe, const int32_t *POS,
                     const int32_t *paint, double g);

/* ---- (4) one block: perform_MI_computation_ACGTN + computeMI_Sprase + fastHadamard fused --- */
/* from_idx[nf], to_idx[nt]: 0-based SNP indices (contiguous ranges for ordinary blocks, arbitrary
 * subsets in SR-only mode, R/computePairwiseMI.R:179-189).  MI_out: nf*nt doubles column-major, host
 * (on_device == 0) or device.  All nf*nt entries are produced, like the reference's MI matrix. */
int ldw_mi_block(ldw_ctx *ctx, const int32_t *from_idx, int64_t nf, const int32_t *to_idx, int64_t nt,
                 int quirk_mode, double *MI_out, int on_device);

/* ---- (5) the a-5 loop: blocks -> sr / lr link tables --------------------------------------- */
typedef struct ldw_mi_params {
    double sr_dist;          /* R/computePairwiseMI.R:47  default 20000 */
    double lr_retain_links;  /* default 1e6 */
    double lr_links_approx;  /* R/computePairwiseMI.R:94-97, computed by the host (R RNG) */
    int32_t sr_only;         /* perform_SR_analysis_only: lr part skipped */
    int32_t quirk_mode;      /* LDW_QUIRK_* */
    int32_t keep_sr;         /* 0: do not materialise sr links (throughput measurement of lr only) */
    int32_t flags;           /* LDW_MI_* bits (0: none) */
} ldw_mi_params;
/* ldw_mi_all_pairs_multi only: the short-range rows STAY on the contexts that computed them — only the long-range table is assembled in
 * ctx[0] — and the short-range model runs over the contexts (7c) */
#define LDW_MI_SR_ROWS_STAY 1

/* blocks[nblocks][4] = (from_s, from_e, to_s, to_e), 1-based inclusive, e.g. this rank's share of
 * make_blocks().  Links are appended to the context's device-resident tables in block order and, within
 * a block, in the reference's row order (R/computePairwiseMI.R:306-310).  reset != 0 clears the tables.
 * Needs the alignment, the weights and the SNP meta data.  The long-range filter is per block (:352-358). */
int ldw_mi_all_pairs(ldw_ctx *ctx, const int32_t *blocks, int64_t nblocks, const ldw_mi_params *p,
                     int reset);
/* The same loop over SEVERAL contexts of this process, one per GPU (the loop it shards is
 * R/computePairwiseMI.R:103-116).  Every context must hold the same alignment, weights and SNP meta data (ldw_set_alignment /
 * ldw_set_weights / ldw_set_snp_meta on each; ldw_hamming_weights_multi shares the weights' own computation).  The block pairs are dealt
 * over the contexts by cost (ldw_deal_blocks), each context runs ldw_mi_all_pairs on its share on a worker thread of its own, and the
 * link tables are assembled in ctx[0] in the caller's block order by peer-to-peer copies.  Afterwards ctx[0] is exactly in the state
 * ldw_mi_all_pairs(ctx[0], all blocks) would have left it in — tables, ldw_block_stats over all nblocks — so everything downstream runs
 * on it unchanged; the other contexts keep their own shares.  The long-range filter is per block (:352-358), so the retained set does
 * not depend on n_ctx.  One failing context fails
 * the call (its message is reported).  owner_out (nblocks, may be NULL) receives the deal; ms_out (10 doubles, may be NULL):
 * [0] deal + slowest pass, [1] gather, [2..9] the pass of contexts 0..7.  n_ctx = 1 is ldw_mi_all_pairs(ctx[0], ..., reset = 1).
 * p->flags & LDW_MI_SR_ROWS_STAY: see (7c). */
int ldw_mi_all_pairs_multi(ldw_ctx **ctx, int n_ctx, const int32_t *blocks, int64_t nblocks, const ldw_mi_params *p,
                           int32_t *owner_out, double *ms_out);
/* The deal alone (host only, no context): owner_out[b] = rank of block b.  A diagonal block pair counts 3.3 times its pairs (its dense
 * short-range band); longest first to the least loaded rank; every rank keeps make_blocks order.  The same deal as ldweaver_amd/dist.py. */
int ldw_deal_blocks(const int32_t *blocks, int64_t nblocks, int n_ranks, int32_t *owner_out);
/* Consecutive long-range-only block pairs of one block row (same from range, to ranges ascending, no pair within sr_dist) run as ONE
 * launch sequence over their concatenated to side, every reference block keeping its own threshold, candidate list and place in the
 * append order.  on != 0 (default): at most max_blocks (2..8; 0 keeps the current value) blocks per span; on = 0: one block at a time.
 * Bits 1 and 2 of on name removed variants and answer LDW_ERR_STATE.  Results do not depend on it. */
int ldw_set_span(ldw_ctx *ctx, int on, int max_blocks);
/* The same loop opened up for blocks that are not contiguous index ranges (SR-only mode drops SNPs
 * without a short-range partner before each block, R/computePairwiseMI.R:179-189):
 * ldw_links_begin(capacity in blocks) ; ldw_mi_block_links(...) per block ; ldw_links_end().
 * The tables are complete after ldw_links_end. */
int ldw_links_begin(ldw_ctx *ctx, int64_t nblocks_capacity);
int ldw_mi_block_links(ldw_ctx *ctx, const int32_t *from_idx, int64_t nf, const int32_t *to_idx, int64_t nt,
                       const ldw_mi_params *p);
int ldw_links_end(ldw_ctx *ctx);
/* which: 0 = short-range, 1 = long-range (after the per-block quantile filter). */
int ldw_links_count(ldw_ctx *ctx, int which, int64_t *n_out);
/* a_out/b_out: 0-based SNP index of the from-side (pos2) and to-side (pos1) SNP; MI_out. capacity in
 * rows; on_device selects the destination space. */
int ldw_links_fetch(ldw_ctx *ctx, int which, int32_t *a_out, int32_t *b_out, double *MI_out,
                    int64_t capacity, int on_device);
/* The table itself, without a copy: DEVICE pointers to the context's own (a, b, MI) columns and the row count; read-only.  Valid until
 * the next call that changes the table (ldw_mi_all_pairs[_multi], ldw_links_begin, ldw_links_import, ldw_sr_reduced_import,
 * ldw_sr_pvalues_multi) and never past ldw_ctx_destroy: synchronise every stream that reads them before either. */
int ldw_links_device_ptrs(ldw_ctx *ctx, int which, const int32_t **a_out, const int32_t **b_out, const double **MI_out,
                          int64_t *n_out);
/* Replace the context's short-range (which = 0) or long-range (1) table by caller data (host or device memory): how the
 * rank that received the other ranks' tables in the multi-GPU gather hands the assembled table to the short-range model,
 * ARACNE and the post-processing entry points below, which work on the context's tables. */
int ldw_links_import(ldw_ctx *ctx, int which, const int32_t *a, const int32_t *b, const double *MI, int64_t n, int on_device);
/* per-block statistics of the last ldw_mi_all_pairs call: n_lr_total, n_lr_kept, n_sr, and the
 * quantile threshold (NaN when no lr links); arrays of length nblocks (may be NULL). */
int ldw_block_stats(ldw_ctx *ctx, int64_t nblocks, int64_t *n_lr_total, int64_t *n_lr_kept,
                    int64_t *n_sr, double *disc_thresh);
/* The index columns of the short-range table from positions alone.  The short-range rows a pass emits for a block pair of contiguous
 * SNP ranges are a pure function of POS, g, sr_dist and the block geometry (R/computePairwiseMI.R:306-333: upper-triangle rows column by
 * column, then the lower ones; pos1 = POS_t[col], pos2 = POS_f[row]), so a multi-GPU gather sends only their MI column and rank 0
 * rebuilds (a, b) here.  blocks: nblocks x 4 (from_s, from_e, to_s, to_e), 1-based inclusive, in the order of the table; a_out / b_out:
 * DEVICE int32 arrays of `capacity` rows (both null: count only); *n_out = rows.  Needs POS ascending (ldw_set_snp_meta). */
int ldw_sr_pairs_fill(ldw_ctx *ctx, const int32_t *blocks, int64_t nblocks, double sr_dist, int32_t *a_out, int32_t *b_out, int64_t capacity, int64_t *n_out);

/* ---- (6) ARACNE — R/io_functions.R:101-164 + src/fintersect.cpp, src/computeMI.cpp:44-77 ---- */
/* flags_out[i] = 1 unless some common neighbour Y of (X,Z) = (chk_pos1[i], chk_pos2[i]) in the full link
 * set has MI(X,Z) < MI(X,Y) and MI(X,Z) < MI(Z,Y).  Positions are compared as exact values. */
int ldw_aracne(ldw_ctx *ctx, const double *chk_pos1, const double *chk_pos2, const double *chk_MI,
               int64_t n_chk, const double *full_pos1, const double *full_pos2, const double *full_MI,
               int64_t n_full, uint8_t *flags_out);

/* ---- (7) short-range model on the device-resident sr table — mergeNsort_sr_links,
 *          R/computePairwiseMI.R:400-495 — and ARACNE on its result.  The table is the one left by
 *          ldw_mi_all_pairs / ldw_links_end; cluster ids come from the paint of ldw_set_snp_meta
 *          (1..nclust, nclust <= 255); len must be integral (integer genome length).  The caller keeps the two
 *          O(1)-sized numerical steps (the log-log OLS fit :428 and the beta MLE :452) and calls, in order: ---- */
/* (:417-424) per cluster c (0-based) and integer len l = 1..S, S = ceil(sr_dist)-1: n_out[c*S + l-1] = number
 * of links with that len touching cluster c+1 (0 < len < sr_dist), and the two order statistics that
 * quantile(type 7, prob) interpolates: ranks floor(h) and ceil(h) of the ascending MI values, h = (n-1)*prob
 * (NaN where n = 0). */
int ldw_sr_len_quantiles(ldw_ctx *ctx, int nclust, double sr_dist, double prob, int32_t S,
                         double *q_lo_out, double *q_hi_out, int64_t *n_out);
/* (:444-452) mean_dist[c*S + l-1] = fitted decay of cluster c+1 looked up BY THE VALUE of len (quirk Q5:
 * NaN beyond the number of distinct lens).  stats_out[c*5 + k] over the links with diff = MI - mean_dist > 0:
 * n, sum diff, sum diff^2, sum log(diff), sum log(1-diff) — reduced in a fixed order. */
int ldw_sr_excess_stats(ldw_ctx *ctx, int nclust, int32_t S, const double *mean_dist, double *stats_out);
/* (:453, :475-490) shape[c*3 + {0,1,2}] = beta shape1, shape2, log B(shape1, shape2).  srp = -log P(X > diff)
 * per link and cluster, maximum over the link's clusters (ties: smaller cluster id), links with
 * srp > srp_cutoff are kept on the device (n_red), and the ARACNE pool = links with a positive excess in
 * some cluster and MI >= min MI kept (n_pool; n_pool_out = NULL: no pool is built, see ldw_sr_pool_build). */
int ldw_sr_pvalues(ldw_ctx *ctx, int nclust, int32_t S, const double *mean_dist, const double *shape,
                   double srp_cutoff, int64_t *n_red_out, int64_t *n_pool_out, double *min_mi_out);
/* kept links in no particular order: row in the sr table (ldw_links_fetch order) and that row's (a, b, MI),
 * clust_c, the first cluster (ascending id) in which the link has a positive excess, whether
 * clust1 != clust2, srp_max. */
int ldw_sr_reduced_fetch(ldw_ctx *ctx, int64_t capacity, int64_t *row_out, int32_t *a_out, int32_t *b_out,
                         double *MI_out, int32_t *clust_c_out, int32_t *first_clust_out, uint8_t *dup_out,
                         double *srp_out);
/* the ARACNE pool: (a, b, MI) of its links */
int ldw_sr_pool_fetch(ldw_ctx *ctx, int64_t capacity, int32_t *a_out, int32_t *b_out, double *MI_out);
/* runARACNE (R/io_functions.R:101-164) for the kept links against the pool, both device resident;
 * flags_out[i] belongs to row_out[i] of ldw_sr_reduced_fetch (after ldw_sr_pvalues) or ldw_lr_reduced_fetch (after
 * ldw_lr_tukey). */
int ldw_aracne_device(ldw_ctx *ctx, int64_t capacity, uint8_t *flags_out);

/* ---- (7b) the same model with the short-range table LEFT on the GPUs that computed it (multi-GPU jobs: SURVEY.md 8(e); the
 *          reference's mergeNsort_sr_links, R/computePairwiseMI.R:400-495, sees one table).  Every rank calls (7) on its own rows; what
 *          travels between ranks is per-group bounds and counts, a small share of the MI column, five sums per block and cluster, the
 *          kept links and the ARACNE pool — not the table (host side: ldweaver_amd/dist_srp.py; protocol and proof of the bound:
 *          BOUNDS.md 10, docs/HISTORY.md 7b). ---- */
/* Rows of the context's table at or above a per-(cluster, len) bound.  lower[c*S + l-1] (host; NaN: send nothing, -inf: every member).  A group's
 * rows are the table rows with that len whose pos1 or pos2 lies in cluster c+1 (a row of two clusters is a member of both, :411-414).
 * cnt_out[(l-1)*nclust + c] (host, len-major) = rows passing, *n_out their sum; mi_out (host or device by on_device, `capacity` doubles;
 * NULL: count only) = their MI values grouped in that order, in no particular order within a group.  mi_out is the caller's buffer
 * and is complete on return.  After ldw_sr_len_quantiles (same nclust, S). */
int ldw_sr_tail_extract(ldw_ctx *ctx, int nclust, int32_t S, const double *lower, int64_t *cnt_out, double *mi_out, int64_t capacity,
                        int on_device, int64_t *n_out);
/* The order statistics of quantile(type 7, prob) per (cluster, len) from the candidates of n_src ranks: mi_src[r] / cnt_src[r] = what
 * ldw_sr_tail_extract gave on rank r (values: host or device by on_device; counts: host), n_total[c*S + l-1] = the group's size over all
 * ranks.  Every row that is NOT among the candidates must lie below every candidate of its group (bounds from ldw_sr_len_quantiles of the
 * ranks: the smallest local lower order statistic is one).  q_lo_out / q_hi_out as ldw_sr_len_quantiles.  *violations_out = groups whose
 * order statistic does not lie among the candidates (NaN there; NULL: such a group is an error).  Needs no table, alignment or meta data. */
int ldw_sr_quantiles_merge(ldw_ctx *ctx, int nclust, int32_t S, double prob, int n_src, const double *const *mi_src,
                           const int64_t *const *cnt_src, const int64_t *n_total, int on_device, double *q_lo_out, double *q_hi_out,
                           int64_t *violations_out);
/* ldw_sr_excess_stats per reference block: the table's rows are those of `nblocks` blocks in order, rows_per_block[b] each (sum = the
 * table's rows); stats_out[(b*nclust + c)*5 + k].  A block's sums depend on its own rows only (64 strips, fixed order), so the sum over
 * all blocks in make_blocks order is bit-identical however the blocks were dealt over ranks. */
int ldw_sr_excess_stats_blocks(ldw_ctx *ctx, int nclust, int32_t S, const double *mean_dist, int64_t nblocks, const int64_t *rows_per_block,
                               double *stats_out);
/* The ARACNE pool of this context's rows for a minimum taken over all ranks (ldw_sr_pvalues with n_pool_out = NULL builds none): rows with a
 * positive excess in some cluster and MI >= min_mi (:489-490); NaN: empty.  Then ldw_sr_pool_fetch. */
int ldw_sr_pool_build(ldw_ctx *ctx, double min_mi, int64_t *n_pool_out);
/* Rank 0: adopt the kept links and the pool of all ranks (host arrays, 0-based from-side / to-side SNP index and MI).  The kept links REPLACE
 * the context's short-range table (rows 0..n_red-1); ldw_aracne_device then answers for them in that order. */
int ldw_sr_reduced_import(ldw_ctx *ctx, int64_t n_red, const int32_t *a, const int32_t *b, const double *MI, int64_t n_pool,
                          const int32_t *pool_a, const int32_t *pool_b, const double *pool_MI);

/* ---- (7c) (7) over the contexts of ONE process after ldw_mi_all_pairs_multi(.., flags = LDW_MI_SR_ROWS_STAY): the protocol of (7b) run by the
 *          library itself (a worker thread per context, exchanges staged through host memory), behind the signatures of (7) — so a single-process
 *          host (R: r_shim/) keeps its three calls and its own fit / optimiser between them.  ctx[0] of that call must be ctx[0] here.  With one
 *          context, or tables that were gathered (no flag), they are (7) on ctx[0] — with the excess sums taken per block when the table's block
 *          structure is known, so that one context and several give the same bits. ---- */
int ldw_sr_len_quantiles_multi(ldw_ctx **ctx, int n_ctx, int nclust, double sr_dist, double prob, int32_t S, double *q_lo_out, double *q_hi_out,
                               int64_t *n_out);
int ldw_sr_excess_stats_multi(ldw_ctx **ctx, int n_ctx, int nclust, int32_t S, const double *mean_dist, double *stats_out);
/* ... and the kept links of ALL contexts end up in ctx[0] (they replace its short-range table, ordered as in the job's table: make_blocks order), with the
 * pool of all contexts: ldw_sr_reduced_fetch / ldw_sr_pool_fetch / ldw_aracne_device on ctx[0] follow as after ldw_sr_pvalues. */
int ldw_sr_pvalues_multi(ldw_ctx **ctx, int n_ctx, int nclust, int32_t S, const double *mean_dist, const double *shape, double srp_cutoff,
                         int64_t *n_red_out, int64_t *n_pool_out, double *min_mi_out);

/* ---- (8) consumers of the link tables, on the device-resident tables ------------------ */
/* Numeric core of analyse_long_range_links (R/lr_analyser.R:72-111): q13_out = quantile(MI, c(.25,.75)) (type 7) of the
 * long-range table, thresholds_out = q3 + (1.5, 3) IQR — or, when fewer than min_links (reference: 5000) links exceed
 * min(thresholds) although the table has that many rows, quantile(MI, 1 - c(4000, 5000)/n) (*fallback_out = 1, the
 * reference's warning).  sr_a / sr_b / sr_mi (host, n_sr_rows >= 0 rows: 0-based from-side / to-side SNP index and MI) is the
 * short-range table the reference reads back from sr_links.tsv (R/lr_analyser.R:67), i.e. the REDUCED set
 * perform_MI_computation returned (srp_max > srp_cutoff, R/computePairwiseMI.R:122,140) — not the raw short-range table.
 * Leaves on the device: the outlier links lr[MI > min(thresholds)] (n_red, table order) and the ARACNE pool
 * rbind(lr, sr)[MI > min(thresholds)] (n_pool, R/lr_analyser.R:106-109).  Then ldw_lr_reduced_fetch / ldw_aracne_device. */
int ldw_lr_tukey(ldw_ctx *ctx, int64_t min_links, const int32_t *sr_a, const int32_t *sr_b, const double *sr_mi,
                 int64_t n_sr_rows, double q13_out[2], double thresholds_out[2], int *fallback_out,
                 int64_t *n_red_out, int64_t *n_pool_out);
/* the outlier links: row in the lr table (ldw_links_fetch order) and that row's (a, b, MI) */
int ldw_lr_reduced_fetch(ldw_ctx *ctx, int64_t capacity, int64_t *row_out, int32_t *a_out, int32_t *b_out, double *MI_out);
/* Numeric core of genomewide_LDMap (R/LDSummaryPlot.R:55-106): pos_vec = sorted unique positions of all links (kept
 * if from < pos < to when a window is given; from = to = 0: genome-wide), symmetric sparse MI matrix over their ranks,
 * block sums with the kernel of .mat(n, reducer) (:176-178), / reducer^2, log10(. + 1e-5), rescaled to [0, 1] (:157-163).
 * reducer = 0: round(length(pos_vec) / 1e3) like the reference.  htm_out: B x B doubles, B = n_pos / reducer (integer
 * division), symmetric; htm_out = NULL only returns the sizes.  reducer <= 1 (the reference's unreduced dense plot) is
 * refused with LDW_ERR_ARG. */
int ldw_ldmap(ldw_ctx *ctx, int32_t reducer, int32_t from, int32_t to, int64_t *n_pos_out, int32_t *reducer_out, int32_t *B_out,
              double *htm_out, int64_t capacity);

/* ---- (8b) CDS variation and SNP paint: estimate_variation_in_CDS (R/estimateCDSDiversity.R:27-123), perform_clustering (:127-148),
 *           painter (:151-210) ------------------------------------------------------------------------------------------------------
 * Variation of every CDS from the resident alignment (ldw_set_alignment or the FASTA route; LDW_ERR_STATE without one).  POS: L (the
 * resident alignment's SNP count) 1-based positions in any order, repeats allowed, each within 1..g; ref_seq: the g characters of the
 * reference (case preserved).  Per SNP the ACGTN_table column is masked by .ACGTN2num's rule (case-sensitive: A/C/G/T rows 0..3, N and '-'
 * row 4, other characters mask nothing).  var_out[j] = sum(snp_var : cds_start[j] <= POS <= cds_end[j]) / (cds_end[j] - cds_start[j] + 1),
 * exact integer sum and one fp64 division (bit-identical to R), NaN when no SNP falls inside (R's NA; a CDS with end < start holds none).
 * Optional outputs (NULL: not written): snp_var_out int64 [L] masked sums; alt_mask_out uint8 [L], bit x set when the masked count of
 * state x (A,C,G,T,N) is > 0; ref_out [L] the reference character of each SNP.  The sorted positions stay on the context for ldw_cds_paint. */
int ldw_cds_variation(ldw_ctx *ctx, const int32_t *POS, int64_t L, const char *ref_seq, int64_t g, const int32_t *cds_start,
                      const int32_t *cds_end, int64_t ncds, double *var_out, int64_t *snp_var_out, uint8_t *alt_mask_out, char *ref_out);
/* painter over the SNPs of the last ldw_cds_variation: paint_out int32 [L] in SNP index order.  label[j] in 1..nclust (nclust <= 255) for the
 * nkept kept CDSs; a SNP takes the largest label of any CDS with cds_start < POS < cds_end (strict), then the 0 runs are filled as painter
 * does from its run table (first run from the right, last recorded run from the left, interior runs split at round((e - b) / 2), half to
 * even).  LDW_QUIRK_REFERENCE leaves a last run of one SNP that differs from its predecessor unrecorded, as the reference's loop does (such
 * a SNP keeps 0 when it is unpainted); LDW_QUIRK_INTENDED records it.  *n_unpainted_out (may be NULL): SNPs left at 0.  LDW_ERR_ARG when no
 * recorded run is painted (no SNP lies strictly inside a kept CDS).  Where the reference stops with an R error — L = 1, no interior 0 run —
 * the paint is returned as it stands. */
int ldw_cds_paint(ldw_ctx *ctx, const int32_t *cds_start, const int32_t *cds_end, const int32_t *label, int64_t nkept, int nclust,
                  int quirk_mode, int32_t *paint_out, int64_t *n_unpainted_out);
/* Host only.  k-means of n values into k clusters at the EXACT optimum of the within-cluster sum of squares (1-D clusters are contiguous in
 * sorted order: a DP over the distinct values with divide-and-conquer rows, O(k n log n)), in place of stats::kmeans(x, k, nstart = 10), which
 * draws from R's unseeded RNG.  Equal values share a cluster; exact cost ties go to the smallest split point.  label_out [n] in 1..k by cluster
 * size, descending (ties: ascending cluster mean), as perform_clustering relabels; *cutoff_out = max(x[label == 1]).  LDW_ERR_ARG for
 * non-finite values, k < 1 or fewer than k distinct values (n = 0 included) ("more cluster centers than distinct data points."). */
int ldw_kmeans_1d(const double *x, int64_t n, int32_t k, int32_t *label_out, double *cutoff_out);
/* Host only, no context and no GPU: the GenBank reader behind parse_genbank_file (R/parseGBK.R), the annotation route the reference's
 * estimate_variation_in_CDS takes (R/estimateCDSDiversity.R:39-47).  One record, plain or gzip, LF / CRLF / CR lines; '<' and '>' are deleted
 * from the whole text first.  Every segment of every feature whose key is exactly "CDS" is one row, in file order: start / end int64,
 * 1-based inclusive (a..b, a, a^b -> [a, b-1]), strand +1 / -1 (complement), feature the 0-based index of its CDS feature.  seq: the ORIGIN
 * sequence (whitespace, digits and "//" removed; IUPAC DNA letters and -+. only; stored UPPER CASE) cut to the range of the single source
 * feature, g bytes.  meta: NUL-terminated strings: the sequence name (/chromosome, /strain or /organism of source), the LOCUS name, the first
 * ACCESSION and the VERSION, then locus_tag, gene and product of each CDS feature ("" when absent).  Errors (LDW_ERR_ARG) name the line:
 * a segment of negative width, a location outside the grammar (remote accession, gap(), one-of(), nested join), no ORIGIN or not exactly one
 * source range ("The GBK file should contain the reference sequence!"), more than one record.  Grammar and divergences: DESIGN.md 17.
 * _probe gives the sizes; _read parses the file again into buffers of at least those sizes (LDW_ERR_SIZE otherwise). */
int ldw_gbk_probe(const char *path, int64_t *n_rows, int64_t *n_features, int64_t *g, int64_t *meta_bytes);
int ldw_gbk_read(const char *path, int64_t rows_cap, int64_t *start, int64_t *end, int8_t *strand, int64_t *feature, int64_t g_cap, char *seq,
                 int64_t meta_cap, char *meta);

/* ---- (9) the tsv files — write.table(x, file, append = T, quote = F, row.names = F, col.names = F, sep = '\t'),
 *          R/computePairwiseMI.R:140 (sr_links.tsv) and :362 (lr_links.tsv); readers R/io_functions.R:32-66 ------------
 * SINGLE WRITER PER PATH: the tsv writers position their workers' writes by offsets computed from the file's size at the start of the call
 * (pwrite), so two writers appending to one path at the same time — two contexts or ranks, or a synchronous call beside a pending
 * ldw_write_links_tsv_begin / ldw_lr_stream_begin on the same file — overwrite each other.  One process appends to lr_links.tsv, as in the
 * reference's serial loop (R/computePairwiseMI.R:103-116). */
#define LDW_COL_INT32 0
#define LDW_COL_INT64 1
#define LDW_COL_DOUBLE 2
/* One double as write.table prints it (R's formatReal, digits = 15: fewest significant digits that reproduce the 15-digit
 * value; fixed notation unless wider than scientific, so 100000 -> "1e+05").  out: >= 48 bytes, NUL-terminated. */
int ldw_format_number(double x, char *out, int capacity);
/* R's `set.seed(seed); sample(n, size)` (1-based, without replacement; Mersenne-Twister, rejection sampling: R >= 3.6 defaults) — the
 * draw behind the 10 % SNP subset of R/computePairwiseMI.R:94-97 (`lr_links_approx`).  n > 1e7 with size <= n / 2 takes R's hashing
 * variant (`sample.int(useHash = TRUE)`, do_sample2: elements re-drawn while they repeat an earlier one), as R itself does.  Host only. */
int ldw_r_sample(uint32_t seed, int64_t n, int64_t size, int64_t *out);
/* nrows x ncols numeric table (host columns of kind LDW_COL_*), tab-separated, no header, appended (append != 0) or
 * truncating; rows are formatted by nthreads host threads (0 = all cores) and written in order.  bytes_out may be NULL. */
int ldw_write_table_tsv(const char *path, int append, int64_t nrows, int ncols, const int32_t *col_kind, const void *const *cols,
                        int nthreads, int64_t *bytes_out);
/* The same with string-table columns as well: a column of kind LDW_COL_STR holds int32 indices; row i prints string
 * col_base[k] + index[i] of the table (strings j at blob[offs[j] .. offs[j + 1]), nstr of them, no NUL needed); an index outside the table
 * is LDW_ERR_ARG.  col_base is read for LDW_COL_STR columns only. */
#define LDW_COL_STR 3
int ldw_write_table_tsv_str(const char *path, int append, int64_t nrows, int ncols, const int32_t *col_kind, const void *const *cols,
                            const int64_t *col_base, const char *blob, const int64_t *offs, int64_t nstr, int nthreads, int64_t *bytes_out);
/* The context's short-range (which = 0) or long-range (1) link table as the reference's MI_df rows `pos1 pos2 clust1 clust2 len MI`
 * (R/computePairwiseMI.R:319-331: pos1 = POS of the to-side SNP, integer columns; clust, len, MI doubles), fetched from the
 * device and formatted by host threads.  An empty table writes nothing, like the reference (:360). */
int ldw_write_links_tsv(ldw_ctx *ctx, int which, const char *path, int append, int nthreads, int64_t *rows_out, int64_t *bytes_out);
/* The same table written BESIDE the caller's next calls: _begin fetches the table from the device (synchronously: the table may be
 * replaced afterwards) and returns while host threads derive, format and write it; _end waits for them and reports rows, bytes and the
 * writer's status.  lr_links.tsv (R/computePairwiseMI.R:362) does not depend on the short-range model that follows it (:119-126), so a job
 * can write it while that model runs.  One asynchronous table per context at a time (_begin, the synchronous call,
 * ldw_set_snp_meta and ldw_ctx_destroy finish a pending one first); _end without _begin returns 0 rows. */
int ldw_write_links_tsv_begin(ldw_ctx *ctx, int which, const char *path, int append, int nthreads);
int ldw_write_links_tsv_end(ldw_ctx *ctx, int64_t *rows_out, int64_t *bytes_out);
/* waits for a pending asynchronous table, discarding its counts (status returned) */
int ldw_tsv_join(ldw_ctx *ctx);
/* lr_links.tsv appended WHILE the pass runs, as the reference appends it block by block (R/computePairwiseMI.R:362).  _begin (before
 * ldw_mi_all_pairs; append = 0 truncates the file first) opens a writer thread on the context; after every finished item of the pass (a
 * block, or a span of blocks) the rows it added to the long-range table — final: the filter is per block (:352-358) — are fetched on a
 * stream of their own, formatted like ldw_write_links_tsv and appended.  The file is at all times a prefix of the complete file in whole
 * blocks; a pass that fails at block k leaves the rows of blocks 0..k-1 (the items already submitted are run to their end first), a killed
 * process those of the items written so far.  _end waits for the writer and reports rows, bytes and the number of blocks whose rows are in
 * the file (any output may be NULL); without _begin it returns zeros.  Single context, single pass: the multi-context gather reorders rows
 * and keeps the table-at-once writer. */
int ldw_lr_stream_begin(ldw_ctx *ctx, const char *path, int append, int nthreads);
int ldw_lr_stream_end(ldw_ctx *ctx, int64_t *rows_out, int64_t *bytes_out, int64_t *blocks_out);

/* ---- (10) the SNP alignment as text — snpdat_to_fa (R/io_functions.R:363-417), generate_Links_SNPS_fasta (:432-460), snps.aln of
 *           write_output_for_gwes_explorer (R/createGWESExplorerOutput.R:23-76) -------------------------------------------------------
 * The k SNP rows snp_idx (0-based, any order, repeats allowed, each in [0, L)) of the resident alignment, every sequence in its original
 * order, states 0..4 printed as A C G T N.  format 0: FASTA records ">name\n" + k characters + "\n"; format 1: the body of write.table's tsv,
 * name + k x ("\t" character) + "\n" (the header line is the caller's).  names: N names, each followed by a NUL (names_bytes in total); a
 * name may not hold '\n'.  The file is appended to (append != 0) or truncated.  The text is rendered on the device and written in chunks of
 * whole records of at most chunk_bytes (<= 0: 64 MiB; a larger record is a chunk of its own) through two pinned buffers that ldw_host_trim
 * gives back.  LDW_ERR_STATE without a resident alignment; LDW_ERR_ARG for an index outside [0, L), k < 1, a name count other than N, a
 * name with a newline, or a path that cannot be opened (the message names the path).  *bytes_out (may be NULL): bytes written. */
int ldw_write_alignment(ldw_ctx *ctx, const char *path, int append, int format, const int32_t *snp_idx, int64_t k, const char *names,
                        int64_t names_bytes, int64_t chunk_bytes, int64_t *bytes_out);

/* ---- (11) the SnpEff step — perform_snpEff_annotations (R/SnpEffAnnotations.R:29-103): a coding-effect predictor and the link join ------
 * ldw_annot_snps: the effect of every SNP pos[i] (1-based) with the A/C/G/T alleles of alt_mask[i] (bit x: state x of A C G T; bit 4, the
 * N / gap state, is ignored) on the CDS features of the reference ref (g characters, any case): seg = nseg x (lo, hi, feature) 1-based inclusive
 * segments, each feature's segments contiguous and in coding order (ascending on +, descending on -), features 0..nfeat-1 in file order;
 * strand[f] = +1 / -1.  rec_out: n x LDW_ANNOT_REC int32 records (effect, impact, feature, right feature, c or distance, codon, ref base, alt
 * base, ref amino acid, alt amino acid, allele, 0); the rule table and the effect codes are DESIGN.md 19.  No alignment is needed.
 * ldw_annot_map: every end of the n links (pos1, pos2) to the one SNP of POS (L positions, any order) at that position; *bad_out = the first end
 * (index e < n: pos1[e], else pos2[e - n]) that matches no SNP or several, or -1.  snp_out (capacity L): the SNP index of every annotation row
 * (the distinct link positions, ascending), *rows_out of them.  The row of every link end stays on the device for ldw_annot_links.
 * ldw_annot_links: the links of the last ldw_annot_map in R's order(key, decreasing = TRUE) (stable, NaN last): perm_out the source row of
 * every sorted link, r1_out / r2_out its annotation rows, pair_out 3 code[r1] + code[r2] (codes per row: 0 sy, 1 ns, 2 ig); top_out the sorted
 * indices of the first max_tophits links that pass detect_top_hits (aracne == 1, pair != syXsy, cds_id[r1] != cds_id[r2], both >= 0),
 * *n_top_out of them. */
#define LDW_ANNOT_REC 12
int ldw_annot_snps(ldw_ctx *ctx, const char *ref, int64_t g, const int32_t *seg, int64_t nseg, const int8_t *strand, int64_t nfeat,
                   const int32_t *pos, const uint8_t *alt_mask, int64_t n, int32_t *rec_out);
int ldw_annot_map(ldw_ctx *ctx, const double *pos1, const double *pos2, int64_t n, const int32_t *POS, int64_t L, int32_t *snp_out,
                  int64_t *rows_out, int64_t *bad_out);
int ldw_annot_links(ldw_ctx *ctx, const double *key, const double *aracne, int64_t n, const int8_t *code, const int32_t *cds_id, int64_t rows,
                    int64_t max_tophits, int64_t *perm_out, int32_t *r1_out, int32_t *r2_out, int8_t *pair_out, int64_t *top_out,
                    int64_t *n_top_out);

/* ---- (12) the plots — make_gwes_plots (R/prepareGWESplots.R:25-126), the lr_gwes.png of analyse_long_range_links (R/lr_analyser.R:113-125),
 *           LD_plot.png of genomewide_LDMap (R/LDSummaryPlot.R:108-127) — rendered on the device, framed and written as PNG by the host.
 * Rules.  Axis range = range of the kept rows widened by 5 % on both sides (a zero-width range by +-0.5 first), shared by all
 * panels; px = min(W-1, (int)floor((x - x0) / (x1 - x0) * W)), py = H-1 - min(H-1, (int)floor((y - y0) / (y1 - y0) * H)), fp64, no fused
 * multiply-add.  A point is the opaque disc of the offsets 4 (dx^2 + dy^2) <= D^2 round its centre pixel, clipped at the panel.  Draw order:
 * layer 0 under layer 1, inside a layer ascending srp_max (ordered = 0) or descending row (ordered != 0: the first row is on top), so a pixel
 * shows the maximum key of the discs that cover it.  Rows with a non-finite x, y or srp_max, or a negative srp_max, are dropped and counted.
 * Colours: srp == NULL: layer_rgb[layer]; else layer 0 = 0xC0C0C0 and layer 1 = the six-stop gradient of t = (srp - lo) / (hi - lo), lo / hi
 * the range of srp over the kept layer-1 rows (hi == lo: t = 0.5). */
#define LDW_PLOT_SR_CLUST 0 /* sr_gwes_clust.png: 2200 x 1200, 1..10 facets with strips, colour bar */
#define LDW_PLOT_SR_COMBI 1 /* sr_gwes_combi.png: 2200 x 1200, one panel, colour bar */
#define LDW_PLOT_LR 2       /* lr_gwes.png: 4800 x 1200, one panel */
#define LDW_PLOT_LDMAP 3    /* LD_plot.png: 5000 x 5250, one square panel under a title */
#define LDW_PLOT_MAX_PANELS 10
#define LDW_PLOT_MAX_TICKS 16
#define LDW_PLOT_MAX_D 41
typedef struct ldw_plot_layout {
    int32_t width, height;                       /* canvas */
    int32_t n_panels, rows, cols;                /* facets laid out like ggplot2::wrap_dims, row-major */
    int32_t panel_w, panel_h;                    /* every panel has this size */
    int32_t panel[LDW_PLOT_MAX_PANELS][4];       /* x, y, w, h of every panel (top-left origin) */
    int32_t strip[LDW_PLOT_MAX_PANELS][4];       /* facet strips (w = 0: none) */
    int32_t cbar[4];                             /* colour bar (w = 0: none) */
    int32_t n_xticks, n_yticks;
    int32_t xtick_px[LDW_PLOT_MAX_TICKS];        /* column of every x tick inside a panel (pixel rule) */
    int32_t ytick_px[LDW_PLOT_MAX_TICKS];        /* row of every y tick inside a panel */
    double xlim[2], ylim[2];                     /* axis range (after the 5 %) */
    double xtick[LDW_PLOT_MAX_TICKS], ytick[LDW_PLOT_MAX_TICKS];   /* 1-2-5 positions, ascending */
} ldw_plot_layout;
typedef struct ldw_plot_opts {
    int32_t kind;             /* LDW_PLOT_* (not LDW_PLOT_LDMAP) */
    int32_t D;                /* disc diameter in pixels, odd, 1..LDW_PLOT_MAX_D; 0 = 11 */
    int32_t ordered;          /* are_srlinks_ordered: row order is the draw order, first row on top (needs srp) */
    int32_t flags;            /* LDW_PLOT_NO_PRECHECK (measurement only: same picture) */
    uint32_t layer_rgb[2];    /* 0xRRGGBB of layer 0 / 1 when srp == NULL */
    int32_t has_hline;        /* one-pixel horizontal line at y = hline_y over the points (widens the y range like a row) */
    uint32_t hline_rgb;
    double hline_y;
} ldw_plot_opts;
#define LDW_PLOT_NO_PRECHECK 1
/* Host only, no context and no GPU.  The figure of `kind` with n_panels facets (1 unless LDW_PLOT_SR_CLUST) for the DATA ranges
 * [x_min, x_max] x [y_min, y_max] (ignored by LDW_PLOT_LDMAP, which has no ticks). */
int ldw_plot_layout_get(int kind, int n_panels, double x_min, double x_max, double y_min, double y_max, ldw_plot_layout *out);
/* Host only: ticks of one axis of `npx` pixels for the data range [lo, hi]: lim_out = the axis range, tick_out / px_out (capacity
 * LDW_PLOT_MAX_TICKS) the 1-2-5 positions inside it and their pixel offset by the pixel rule (flip != 0: the y axis, row 0 on top). */
int ldw_plot_ticks(double lo, double hi, int npx, int flip, double lim_out[2], double *tick_out, int32_t *px_out, int32_t *n_out);
/* Host only: 8-bit RGB, non-interlaced PNG of rgb[height][width][3]; level 0..9 is zlib's (-1: 1). */
int ldw_png_write(const char *path, const uint8_t *rgb, int32_t width, int32_t height, int level, int64_t *bytes_out);
/* The scatter figure of n rows: x, y doubles, srp doubles (NULL: fixed colours), layer uint8 0 / 1 (NULL: all 1), panel uint8 in
 * [0, n_panels) (NULL: all 0), host or device memory (host columns pass through a device buffer of constant size in chunks of 2^20 rows; the
 * row-order key also keeps a device copy of the srp column, which the colour pass reads by row).  panel_label[n_panels] (may be NULL) is
 * printed on the strips.  The figure goes to png_path (may be NULL) and / or rgb_out (may be NULL: height x width x 3 bytes of the layout's
 * canvas).  *dropped_out (may be NULL): rows dropped.  n = 0 gives the frame over the unit ranges. */
int ldw_plot_scatter(ldw_ctx *ctx, const double *x, const double *y, const double *srp, const uint8_t *layer, const uint8_t *panel, int64_t n,
                     int on_device, const ldw_plot_opts *opts, int n_panels, const int32_t *panel_label, const char *png_path, uint8_t *rgb_out,
                     int64_t *dropped_out);
/* The same from the context's own state, nothing copied to the host: the kept links of ldw_sr_pvalues (which = 0: x = len from POS and g of
 * ldw_set_snp_meta by the circ_len rule, y = MI, srp = srp_max, panel = rank of clust_c among the clust_c present, LDW_PLOT_SR_CLUST or
 * _COMBI) or of ldw_lr_tukey (which = 1: LDW_PLOT_LR, fixed colours).  use_aracne != 0: layer = the flags of the last ldw_aracne_device
 * (LDW_ERR_STATE if it has not run since the kept links last changed: the context keeps track); 0: every row in layer 1.  LDW_ERR_STATE also
 * without SNP meta data and when the kept links are those of the other table. */
int ldw_plot_links(ldw_ctx *ctx, int which, int use_aracne, const ldw_plot_opts *opts, const char *png_path, uint8_t *rgb_out, int64_t *dropped_out);
/* LD_plot.png: htm (B x B doubles in [0, 1], host or device) through the 2056-colour ramp white, #E1B9B4, #AE452C, #802418 (index
 * min(floor(v * 2056), 2055); non-finite: 0), nearest neighbour, row 0 at the bottom; title (may be NULL) above it. */
int ldw_plot_heatmap(ldw_ctx *ctx, const double *htm, int32_t B, int on_device, const char *title, const char *png_path, uint8_t *rgb_out);
/* ldw_ldmap and its picture in one call: the map is rendered from the device copy; htm_out (may be NULL) as in ldw_ldmap. */
int ldw_plot_ldmap(ldw_ctx *ctx, int32_t reducer, int32_t from, int32_t to, const char *title, const char *png_path, int64_t *n_pos_out,
                   int32_t *reducer_out, int32_t *B_out, double *htm_out, int64_t capacity);

/* The "xy" figures: c<i>_fit.png of perform_MI_computation (R/computePairwiseMI.R:430-440) — black points, a red polyline over them — and
 * CDS_clustering.png of estimate_variation_in_CDS (R/estimateCDSDiversity.R:212-220) — points coloured by class.  The rules are those of the scatter
 * figures where they apply (axis range, pixel rule, opaque disc, grid lines, font).  Kept points: x, y finite (the others are dropped and counted); cls ==
 * NULL: class 0; a row, kept or dropped, with cls >= n_classes refuses the call (LDW_ERR_ARG) before anything is drawn.  Draw order = row order, the LATER
 * row on top: a pixel shows the class of the largest row whose disc covers it.  Line: segment i joins vertices i and i + 1 and exists iff both are finite
 * (x and y); a finite vertex with no finite neighbour is a disc of diameter line_w; every segment is the opaque capsule of width line_w between the two
 * vertices' centre pixels by the network plot's integer rule 4 D2 <= w^2 (below), drawn over the points and clipped at the panel.  Axis range: that of the
 * kept points and the finite vertices together, widened by 5 % (nothing kept: [0, 1]).  line_x / line_y are HOST arrays of at most 2^17 vertices in
 * drawing order (n_line may be 0); x, y, cls are host or device memory (on_device), host columns passing through the chunk buffer of ldw_plot_scatter. */
#define LDW_PLOT_FIT 4   /* c<i>_fit.png: 2200 x 1200, one panel under a title; black points, a red line over them */
#define LDW_PLOT_CDS 5   /* CDS_clustering.png: 2200 x 1200, one panel, points coloured by class, a legend on the right */
#define LDW_PLOT_MAX_CLASSES 10
typedef struct ldw_plot_xy_opts {
    int32_t kind;            /* LDW_PLOT_FIT or LDW_PLOT_CDS */
    int32_t D;               /* disc diameter, odd, 1..LDW_PLOT_MAX_D; 0 = 11 */
    int32_t n_classes;       /* 1..LDW_PLOT_MAX_CLASSES */
    uint32_t class_rgb[LDW_PLOT_MAX_CLASSES];
    int32_t line_w;          /* polyline width in pixels, 1..1024; 0 = 5 (nominal, like D) */
    uint32_t line_rgb;
} ldw_plot_xy_opts;
/* Host only: ldw_plot_layout_get for the xy figures (kind LDW_PLOT_FIT or LDW_PLOT_CDS; n_panels must be 1).  ldw_plot_layout_get itself keeps to the
 * kinds 0..3. */
int ldw_plot_xy_layout_get(int kind, int n_panels, double x_min, double x_max, double y_min, double y_max, ldw_plot_layout *out);
/* The figure: the panel rendered on the device; then, by the host, the frame, the tick labels, xlab under and ylab beside the panel, for LDW_PLOT_FIT the
 * title above it and for LDW_PLOT_CDS the legend "Cluster" with one swatch per class (title, xlab, ylab may be NULL).  The figure goes to png_path (may be
 * NULL) and / or rgb_out (may be NULL: 1200 x 2200 x 3 bytes).  *dropped_out (may be NULL): rows dropped. */
int ldw_plot_xy(ldw_ctx *ctx, const double *x, const double *y, const uint8_t *cls, int64_t n, int on_device, const double *line_x, const double *line_y,
                int64_t n_line, const ldw_plot_xy_opts *opts, const char *title, const char *xlab, const char *ylab, const char *png_path, uint8_t *rgb_out,
                int64_t *dropped_out);

/* The network plot of create_network (R/createNetworkPlot.R:120-139).  Its edges are CAPSULES — the pixels within w / 2 of a segment — blended
 * over a white canvas in list order.  Pixels and endpoints are integer points; with D2 the squared distance from a pixel to the segment (to the nearer end
 * where the projection falls outside it), the pixel is covered iff 4 D2 <= w^2, evaluated exactly in 64-bit integers; a covered pixel takes, per channel,
 * c = (c (255 - alpha) + colour alpha + 127) / 255.  Limits (LDW_ERR_ARG beyond them): canvas 1..8192 each way, endpoint coordinates in -8192..16383 (they
 * may lie outside the canvas and may coincide: a disc), w in 1..1024, alpha in 1..255, at most 2^17 capsules (8192 edges of 16 segments: the binning
 * tests every capsule against every 32 x 32 tile, so its work is tiles x capsules). */
typedef struct ldw_capsule {
    int32_t x0, y0, x1, y1;   /* the segment's ends */
    int32_t w;                /* width in pixels */
    uint32_t rgb;             /* 0xRRGGBB */
    int32_t alpha;            /* 1..255 */
} ldw_capsule;
/* The figure: the capsules rendered on the device; then, by the host, a white bordered box with node_names[k] centred on (node_xy[2k], node_xy[2k + 1]) for
 * every node, the title (may be NULL) centred at the top and, for n_legend > 0, the legend "Num_Links" at the bottom with one swatch legend_rgb[k] and value
 * legend_value[k] each, in the 5 x 7 font at text_scale (1..64).  The figure goes to png_path (may be NULL) and / or rgb_out (may be NULL: H x W x 3 bytes).
 * boxes_out (may be NULL, (n_nodes + 2) x 4 int32): x, y, w, h of what the host drew over the raster — the node boxes, the title, the legend (w = 0: none);
 * a box may reach past the canvas. */
int ldw_plot_network(ldw_ctx *ctx, const ldw_capsule *caps, int64_t n_caps, int32_t W, int32_t H, const int32_t *node_xy, const char *const *node_names,
                     int32_t n_nodes, const char *title, const int32_t *legend_value, const uint32_t *legend_rgb, int32_t n_legend, int32_t text_scale,
                     const char *png_path, uint8_t *rgb_out, int32_t *boxes_out);
/* The tanglegram of create_tanglegram (R/createTanglegram.R): gene-pair links between two genome bars.  The links are capsules, drawn over white
 * exactly as ldw_plot_network draws them (same coverage test, same blend, list order).  Then every RECTANGLE — the half-open pixel box [x0, x1) x [y0, y1),
 * clipped to the canvas — is painted OPAQUE over that raster in list order: a pixel takes the colour of the last rectangle that covers it.  An empty rectangle
 * (x0 = x1 or y0 = y1) paints nothing.  Limits (LDW_ERR_ARG beyond them, before anything runs on the device): those of the capsules; at most 2^16 rectangles,
 * their coordinates in -8192..16383, x1 >= x0 and y1 >= y0, rgb <= 0xFFFFFF. */
typedef struct ldw_rect {
    int32_t x0, y0, x1, y1;   /* half-open */
    uint32_t rgb;             /* 0xRRGGBB, opaque */
} ldw_rect;
/* The figure: capsules and rectangles rendered on the device; then, by the host in the 5 x 7 font at text_scale (1..64), labels[k] read UPWARDS from its
 * anchor (label_xy[2k], label_xy[2k + 1]) = the bottom-left corner of the turned text (7 text_scale wide, as high as the text is long), and the title (may be
 * NULL) centred at the top.  The host makes no layout decisions: an empty label draws nothing.  The figure goes to png_path (may be NULL) and / or rgb_out (may
 * be NULL: H x W x 3 bytes).  boxes_out (may be NULL, (n_labels + 1) x 4 int32): x, y, w, h of what the host drew — the labels, then the title (w = 0: none; an
 * empty label reports its anchor); a box may reach past the canvas. */
int ldw_plot_tanglegram(ldw_ctx *ctx, const ldw_capsule *caps, int64_t n_caps, const ldw_rect *rects, int64_t n_rects, int32_t W, int32_t H,
                        const int32_t *label_xy, const char *const *labels, int32_t n_labels, const char *title, int32_t text_scale, const char *png_path,
                        uint8_t *rgb_out, int32_t *boxes_out);

/* ---- (13) numeric link tables read on the device — the readers of R/io_functions.R:32-66 (read_LongRangeLinks, read_ShortRangeLinks), and through them
 *           the file inputs of genomewide_LDMap (R/LDSummaryPlot.R), analyse_long_range_links (R/lr_analyser.R) and make_gwes_plots -----------------------
 * A text file, plain or gzip (read with zlib), no header, ONE separator byte ('\t' or ' '), every cell a number.  Lines end at '\n'; one '\r' before it is
 * stripped; empty lines are skipped; the last line need not end in a newline; a line may hold at most 2^20 bytes.  A number is: an optional sign, digits
 * with an optional '.' and more digits (at least one digit in all), an optional exponent (e or E, optional sign, digits) — or one of the tokens NA NaN nan
 * (NaN) Inf inf -Inf -inf.  No hex, no separators of thousands, no quotes, no blanks round a cell.  The value of a cell is the correctly rounded double of
 * its decimal text (Python's float()): cells with at most 19 significant digits, a mantissa <= 2^53 and a decimal exponent in [-22, 22] are converted on
 * the device by one fp64 operation, all others ("slow cells") by the host's strtod from the chunk it still holds — they cost time, never a bit.
 * Refusals (LDW_ERR_ARG, ldw_last_error() names the file, the 1-based physical line and the 1-based column; the earliest bad line of the file wins, and
 * inside it the leftmost fault): a cell that is not a number, a line that ends before its ncols-th field (column = the first missing field), a line with
 * more fields (column = ncols + 1), a line that is too long.  A file without rows is no error.  Row order is file order.  Host memory is O(chunk). */
/* Host only, no context: the fields of the first non-empty line (0 for a file without one) and whether the file is gzip (gz_out may be NULL). */
int ldw_tsv_probe(const char *path, int sep, int32_t *ncols_out, int32_t *gz_out);
/* Parses the file into the context's columns (ncols in 1..16), replacing those of the last call, in chunks of chunk_bytes (0: 64 MiB; at most 2^30) read
 * through two pinned buffers that ldw_host_trim gives back.  *rows_out rows; *slow_cells_out cells the host converted; bit k of *int_cols_mask_out: every
 * cell of column k was a plain integer literal [+-]?[0-9]+ (0 for a file without rows).  Any output may be NULL.  After a refusal the context holds no
 * table (rows = 0) and works on. */
int ldw_tsv_read(ldw_ctx *ctx, const char *path, int sep, int32_t ncols, int64_t chunk_bytes, int64_t *rows_out, int64_t *slow_cells_out,
                 uint32_t *int_cols_mask_out);
/* The table itself, without a copy: a DEVICE pointer to the context's own columns, doubles, column k at device_ptr + k * stride (NULL when rows = 0);
 * read-only.  Valid until the next ldw_tsv_read and never past ldw_ctx_destroy: synchronise every stream that reads them before either, as for
 * ldw_links_device_ptrs.  LDW_ERR_STATE before the first ldw_tsv_read. */
int ldw_tsv_columns(ldw_ctx *ctx, const double **device_ptr_out, int64_t *rows_out, int32_t *ncols_out, int64_t *stride_out);
/* one column (0-based) copied out: dst holds `capacity` >= rows doubles, host or device memory */
int ldw_tsv_fetch(ldw_ctx *ctx, int32_t col, double *dst, int64_t capacity, int on_device);
/* Positions for a context WITHOUT an alignment — a directory that holds the link files of an earlier job and nothing else: POS[L] (any order, repeats
 * allowed, like snp.dat$POS) and the genome length g (0: not known; ldw_plot_links(which = 1), which takes len from POS and g, then answers LDW_ERR_STATE).
 * What the context held of an alignment — states, weights, r, uqe, paint — and both link tables are dropped.  Enough for ldw_links_load, ldw_links_import,
 * ldw_ldmap / ldw_plot_ldmap, ldw_lr_tukey, ldw_lr_reduced_fetch, ldw_aracne_device and ldw_plot_links(which = 1); entry points that need the alignment,
 * the weights, uqe or the paint (the MI pass, the short-range model, the tsv writers, ...) keep answering LDW_ERR_STATE until ldw_set_alignment. */
int ldw_set_positions(ldw_ctx *ctx, const int32_t *POS, int64_t L, double g);
/* The columns of the last ldw_tsv_read become the context's short-range (which = 0) or long-range (1) table, exactly as ldw_links_import(on_device = 1)
 * would install it, all on the device: rows whose min_len_col value is below min_len are dropped (min_len_col = -1: none; the reference's `len < sr_dist`
 * drop of long-range files; a NaN stays, as in R); pos1_col maps to the to-side SNP index and pos2_col to the from-side one by the positions of
 * ldw_set_snp_meta or ldw_set_positions, the FIRST SNP at a position; mi_col is the MI column.  Refused (LDW_ERR_ARG, with the file, line and column of the
 * first such row that stays): a position that is not an integer, does not fit in 32 bits, or is no SNP's.  flags: 0.  *n_out (may be NULL): rows installed. */
int ldw_links_load(ldw_ctx *ctx, int which, int32_t pos1_col, int32_t pos2_col, int32_t mi_col, int32_t min_len_col, double min_len, int32_t flags,
                   int64_t *n_out);

/* ---- (14) annotated link files searched on the device — grep(gene, pos1_ann / pos2_ann) of create_network_for_gene (R/createNetworkPlot.R:169-290) over
 *           sr_links_annotated.tsv / lr_links_annotated.tsv of perform_snpEff_annotations ------------------------------------------------------
 * The file: a tab-separated table with ONE header line, plain or gzip, at most 16 columns, its lines under the rules of (13).  The columns pos1, pos2, len,
 * ARACNE, MI (numbers under the grammar and the value rule of (13)) and pos1_ann, pos2_ann, links (byte strings, possibly empty, without a tab) are found BY
 * NAME in the header; every other column is neither parsed nor searched.  An ARACNE cell may also be TRUE or FALSE, read as 1 and 0: the long-range file
 * holds a logical column.  The needles: n in 1..1024 byte strings of 1..255 bytes, needle j = needles[needle_off[j] .. needle_off[j + 1]).  A row is KEPT
 * iff some needle occurs, byte for byte and case sensitive (grep(fixed = TRUE): no regular expressions), inside the field pos1_ann or inside the field
 * pos2_ann — never across a tab — and, with LDW_GREP_DROP_SYXSY, its links field is not exactly "syXsy", and, with LDW_GREP_DROP_INDIRECT, its ARACNE
 * value equals 1.
 * Refused (LDW_ERR_ARG; the message names the file, the 1-based physical line and the 1-based column; the earliest bad line wins, inside it the leftmost
 * fault): a header without one of the eight names (column = fields + 1) or with one of them twice, or with more than 16 fields; a row with fewer (column = the
 * first missing field) or more (column = fields + 1) fields than the header; a cell of the five numeric columns that is not a number; a line over 2^20 bytes;
 * a file without a header line; n or a needle's length out of range.
 * Host memory is O(chunk + kept rows).  Device memory is O(chunk + kept rows of a chunk): the chunk's image, 4 bytes per row of the chunk (its row starts),
 * and one record of 96 + 8 ceil(n / 64) bytes per kept row — room for 16384 at first; a chunk that keeps more is searched once more with room for all its rows —
 * in grow-only buffers that ldw_ctx_destroy frees (ldw_host_trim releases the records and the last result). */
#define LDW_GREP_DROP_SYXSY 1
#define LDW_GREP_DROP_INDIRECT 2
/* Searches the file in chunks of chunk_bytes (0: 64 MiB; at most 2^30) through the pinned buffers of ldw_tsv_read.  The kept rows stay with the context until
 * the next call: *rows_out their count, *text_bytes_out the bytes of their three strings together, *data_rows_out the data rows of the file (any may be NULL). */
int ldw_links_grep(ldw_ctx *ctx, const char *path, const uint8_t *needles, const int32_t *needle_off, int32_t n_needles, int32_t flags, int64_t chunk_bytes,
                   int64_t *rows_out, int64_t *text_bytes_out, int64_t *data_rows_out);
/* The kept rows of the last ldw_links_grep, in file order, into host arrays: row_out[rows] the 0-based index among the data rows; num_out[rows][5] = pos1, pos2,
 * len, ARACNE, MI; mask_out[rows][ceil(n / 64)]: bit j & 63 of word j / 64 set iff needle j occurs in either field; text_out / text_off_out[3 rows + 1]: string
 * 3 i + k of row i (k = 0 pos1_ann, 1 pos2_ann, 2 links) = text_out[text_off_out[3 i + k] .. text_off_out[3 i + k + 1]).  LDW_ERR_SIZE when capacity < rows or
 * text_capacity < the text bytes; LDW_ERR_STATE without a result. */
int ldw_links_grep_fetch(ldw_ctx *ctx, int64_t capacity, int64_t text_capacity, int64_t *row_out, double *num_out, uint64_t *mask_out, uint8_t *text_out,
                         int64_t *text_off_out);

/* ---- (15) the tree view — view_tree (R/preptrees.R): a tree over bands of alleles and metadata, rendered on the device ----------------------
 * The tree is a list of BARS: axis-aligned, half-open rectangles [x0, x1) x [y0, y1) in 1/16 pixel relative to the panel's top-left corner, x1 > x0 and
 * y1 > y0, one per branch and one per connector.  A bar adds to every panel pixel its overlap area with that pixel in units of 1/256 pixel (0..256); a
 * pixel's ink is min(sum, 256) and every channel (255 (256 - ink) + colour ink + 128) >> 8 over white.  Bars are clipped to the panel.  The sums are
 * integers: the picture does not depend on the order of the bars or of the adds.
 * The BANDS: levels[n_bands][n_tips] (uint8), band r drawn into band_rect[4 r ..] = x, y, w, h (canvas pixels) with the colours palette[256 r + level]
 * (0xRRGGBB).  In units where tip i spans [i w, (i + 1) w) and pixel column p spans [p n_tips, (p + 1) n_tips), the overlaps ov of a column with the tips
 * sum to n_tips and every channel is (sum of ov c[level] + n_tips / 2) / n_tips in 64-bit integers; all rows of a band repeat that line.
 * Limits (LDW_ERR_ARG beyond them, before anything runs on the device): at most 2^23 bars (checked first), coordinates within +-2^20; canvas 1..8192 each
 * way; the panel and every band non-empty and inside the canvas, no band overlapping the panel or another band; at most 1024 bands, 2^24 tips and 2^31
 * levels in all. */
typedef struct ldw_bar {
    int32_t x0, y0, x1, y1;
} ldw_bar;
/* The figure: a white canvas W x H, the bars in bar_rgb inside panel = x, y, w, h, the bands; then, by the host in the 5 x 7 font at text_scale (1..64):
 * band_label[r] (may be NULL, entries may be NULL or empty) right-aligned 2 text_scale pixels left of band r and centred on its height; title (may be NULL)
 * centred at the top; two legends, legend k with its top-left corner at legend_xy[2 k], legend_xy[2 k + 1]: legend_title[k] over legend_n[k] (0..256; 0: no
 * legend) rows of a square swatch and a label, the entries of legend 1 following those of legend 0 in legend_label / legend_rgb.  The figure goes to
 * png_path (may be NULL) and / or rgb_out (may be NULL: H x W x 3 bytes).  boxes_out (may be NULL, (n_bands + 3) x 4 int32): x, y, w, h of what the host
 * drew — the band labels, the title, the two legends (w = 0: none); a box may reach past the canvas.  The host does not keep its text off the panel or the
 * bands: the caller's layout does. */
int ldw_plot_tree(ldw_ctx *ctx, int32_t W, int32_t H, const int32_t *panel, const ldw_bar *bars, int64_t n_bars, uint32_t bar_rgb, const uint8_t *levels,
                  int64_t n_tips, const uint32_t *palette, const int32_t *band_rect, int32_t n_bands, const char *const *band_label, const char *title,
                  const char *const *legend_title, const int32_t *legend_n, const char *const *legend_label, const uint32_t *legend_rgb,
                  const int32_t *legend_xy, int32_t text_scale, const char *png_path, uint8_t *rgb_out, int32_t *boxes_out);

/* ---- (16) a neighbour-joining tree built on the device — the tree view_tree otherwise reads from a file -----------------------------------
 * Nodes 0 .. n-1 are the tips, node n + s is made by join s (s = 0 .. n-4) and node 2n-3 is the root, on which the last three nodes hang: the tree is
 * unrooted with a trifurcation.  dist NULL: the resident alignment, d(i, j) = the number of SNPs at which sequences i and j differ under the five-state
 * rule (L - shared of ldw_hamming_weights), and n must be its number of sequences.  Otherwise dist is a HOST n x n fp64 matrix, checked on the device
 * before any join runs: finite, symmetric bit for bit, zero diagonal; its row sums start as r_i = d(0, i) + d(1, i) + ... in that order.  Every join is
 * IEEE fp64 without fused multiply-adds, operation by operation as DESIGN.md 26 states it, ties between equal Q going to the smallest (smaller node id,
 * larger node id): the result is a function of the matrix alone.  parent_out[2n-2]: the parent of every node, -1 at the root; length_out[2n-2]: the branch
 * to the parent, raw (it may be negative), in the matrix's unit — differing SNP columns for the alignment; 0 at the root.
 * LDW_ERR_STATE: dist NULL and no alignment resident.  LDW_ERR_ARG: n < 3, n not the alignment's sequence count, a bad matrix, a null output.  The call
 * holds n x n x 8 bytes of device memory (beside the Hamming stage's, released before the joins) and gives it back; the alignment, the weights, the SNP
 * metadata and the link tables of the context stay as they are. */
int ldw_nj_tree(ldw_ctx *ctx, const double *dist, int64_t n, int32_t *parent_out, double *length_out);

/* Bootstrap support of that tree.  mult[B][L] (HOST, a row per replicate): how often replicate b holds SNP column a of the resident
 * alignment, 0 <= mult <= 63 and every row's sum < 2^27 — L draws with replacement for the bootstrap proper, 0 / 1 for a jackknife, any other weighting.
 * Replicate b's distance is d_b(i, j) = the sum of mult[b][a] over the columns a at which sequences i and j differ (five-state rule), its tree the tree
 * ldw_nj_tree would build of that matrix, bit for bit.  parent_out / length_out [2n-2]: the tree of the alignment itself, exactly ldw_nj_tree's.
 * support_out[2n-2]: for a join node u = n .. 2n-4 (the n - 3 internal edges of the unrooted tree) the number of replicates whose tree has a join node
 * that splits the tips into the same two sets as u does; -1 at the tips and at the root.  rep_parent_out [B][2n-2] and rep_length_out [B][2n-2] (each
 * may be NULL): the replicates' trees, for tests and for callers who build a consensus of their own.  Splits are compared on the device by a pair of
 * 64-bit sums of per-tip keys: two different splits are taken for one with probability at most B (n-3)^2 2^-128.
 * The replicates' trees are joined R side by side (R = min(B, 16, 4 GiB / 8 n^2), at least 1; LDW_NJ_BATCH=k in the environment, read at every call,
 * forces R = k: a test hook); no result depends on R.  Nothing is read back between the joins.  ldw_ctx_last_timing afterwards, summed over the
 * replicates: [0] joins, [1] multiplicities + digits + GEMMs + fills, [2] split sums + look-ups, [3] their sum.
 * Refused before any join, the context staying usable — LDW_ERR_STATE: no alignment resident.  LDW_ERR_ARG: n not the alignment's sequence count,
 * n < 3, B < 1, mult or one of the three first outputs NULL, a multiplicity outside 0..63, a row sum >= 2^27.  The call holds the Hamming stage's
 * working memory, R n x n x 8 bytes and, with a replicate output, B (2n-2) x 12 bytes on the device and gives them back; the alignment, the weights,
 * the SNP metadata and the link tables of the context stay as they are. */
int ldw_nj_bootstrap(ldw_ctx *ctx, const int32_t *mult, int64_t B, int64_t n, int32_t *parent_out, double *length_out, int32_t *support_out,
                     int32_t *rep_parent_out, double *rep_length_out);

/* ---- (17) maximum parsimony on a given tree: what a SNP, and a pair of SNPs, does along the branches ---------------------------------------
 * The tree: parent[nodes] (HOST), parent[0] = -1 and 0 <= parent[v] < v otherwise — the numbering of the Python Tree; a node may have any number of
 * children, one included.  tip_seq[nodes] (HOST): for a node without children the 0-based sequence of the resident alignment it stands for, -1 for a node
 * with children; the tree may hold a subset of the sequences in any order, none of them twice.
 * A node's set is a mask of the states 0..4 (A, C, G, T, N).  Tips: under gap_mode 0 a tip in state N gets the set {A, C, G, T}, a wildcard that costs
 * nothing, any other tip {s}; under gap_mode 1 every tip gets {s} and N is a fifth state.  Up pass (Hartigan's rule; Fitch's for two children), v from
 * nodes-1 down to 0: for a node with children, c(s) = the children whose set holds s, K = max c, set(v) = {s : c(s) = K}, score += arity(v) - K.  Down pass:
 * state(0) = the lowest state of set(0); for v = 1 .. nodes-1, state(v) = state(parent(v)) where set(v) holds it, else the lowest state of set(v); branch v
 * changes where state(v) != state(parent(v)).  The changes of a SNP number its score, which is the least number any reconstruction needs.
 * ldw_tree_parsimony: for every SNP of the alignment, score_out[L] and min_changes_out[L] = the distinct states at the tree's tips minus one, floored at 0
 * (N not counted under gap_mode 0); homoplasy = score - min_changes.
 * SNPs are processed in chunks whose node sets (nodes bytes per SNP) stay within 1 GiB; LDW_PARS_CHUNK=k in the environment, read at every call, forces
 * chunks of k SNPs: a test hook, no result depends on it.  ldw_ctx_last_timing afterwards: [0] the passes, [1] the gathers of the tips' states, [2] what
 * follows them (copies, transposes, pairs), [3] their sum.
 * Refused on the host before anything is launched, the context staying usable — LDW_ERR_STATE: no alignment resident.  LDW_ERR_ARG: nodes < 2 or fewer than
 * two tips; parent[0] != -1 or a parent[v] outside [0, v); a childless node whose tip_seq is outside [0, N) or names a sequence another tip names; a node
 * with children whose tip_seq is not -1; gap_mode other than 0 or 1; a SNP index outside [0, L); k or K < 1; a null pointer.  The message names the node or
 * the index.  Every call takes its working memory and gives it back; the alignment, the weights, the SNP metadata and the link tables stay as they are. */
int ldw_tree_parsimony(ldw_ctx *ctx, const int32_t *parent, const int32_t *tip_seq, int64_t nodes, int32_t gap_mode, int32_t *score_out,
                       int32_t *min_changes_out);
/* The reconstruction itself: node_state_out[k][nodes] (HOST), row i the state 0..4 of every node for SNP snp_idx[i] (HOST, 0-based, any order, repeats
 * allowed: equal rows). */
int ldw_tree_states(ldw_ctx *ctx, const int32_t *parent, const int32_t *tip_seq, int64_t nodes, int32_t gap_mode, const int32_t *snp_idx, int64_t k,
                    uint8_t *node_state_out);
/* Pairs of SNPs (pair_a[K], pair_b[K], HOST; a == b and repeated pairs allowed): changes_a_out[K] and changes_b_out[K] the branches on which each SNP
 * changes (= its score), co_out[K] the branches v >= 1 on which both do.  Only the distinct SNPs named go through the passes; each leaves a bitmap of
 * its changed branches (nodes / 8 bytes per distinct SNP, held for the call) and a pair is the popcount of the AND of two. */
int ldw_tree_cochanges(ldw_ctx *ctx, const int32_t *parent, const int32_t *tip_seq, int64_t nodes, int32_t gap_mode, const int32_t *pair_a,
                       const int32_t *pair_b, int64_t K, int32_t *changes_a_out, int32_t *changes_b_out, int32_t *co_out);

/* ---- (18) the lineage check for links: clusters of the sequences, and the MI of listed SNP pairs inside them --------------------------------
 * ldw_seq_clusters: single-linkage clusters of the sequences of the resident alignment.  Sequences i and j are neighbours at threshold t iff
 * L - shared(i, j) < t, the predicate of ldw_hamming_weights (strict, in differing SNP columns under the five-state rule); a cluster is a connected
 * component of that graph.  thresh[n_thresh] (HOST, 1..16 of them, each >= 0) are served from ONE Hamming GEMM.  labels_out[n_thresh][N] (HOST): clusters
 * are numbered 0, 1, ... in the order of their smallest member, so a row is a function of the alignment and t alone; n_clusters_out[n_thresh].  t = 0 gives
 * N singletons, t = 1 joins identical sequences, t > L gives one cluster; a larger t only merges clusters.  The components are found by rounds of hooking
 * onto roots and pointer jumping over a bit adjacency matrix; the host reads one word back per round.  ldw_ctx_last_timing afterwards: [0] the rounds,
 * [1] the GEMM and whatever else ran in front of them, [2] the rounds taken (of the threshold that took most), [3] the sum of [0] and [1].
 * LDW_ERR_STATE: no alignment resident.  LDW_ERR_ARG: n_thresh outside 1..16, a negative threshold, a null pointer.  The call runs on the context's stream,
 * takes the Hamming stage's working memory and N x Npad / 8 bytes per threshold and gives them back; the alignment, the weights, the SNP metadata and the
 * link tables stay as they are. */
int ldw_seq_clusters(ldw_ctx *ctx, const int32_t *thresh, int32_t n_thresh, int32_t *labels_out, int32_t *n_clusters_out);
/* ldw_links_stratified: per cluster of a partition of the sequences, the joint tables and the weighted MI of the SNP pairs (pair_a[i], pair_b[i]), i < K
 * (HOST, 0-based; a == b and repeated pairs allowed).  labels[N] (HOST): the cluster 0 .. C-1 of every sequence, or -1 for a sequence left out of
 * everything; a cluster without a member is legal: its tables, MI and flags are 0.  Needs the alignment and the weights (ldw_set_weights), not the SNP
 * metadata; the weights are the resident ones, not re-estimated per cluster.  For cluster c and pair (a, b):
 *   counts[X][Y]  the members of c in state X at a and Y at b; fixed[X][Y] the sum of their V_s = round(fl(sqrt w_s)^2 2^F), F in *frac_bits_out as with
 *                 ldw_joint_tables; both exact.  counts_out / fixed_out [K][C][25] (HOST) may both be NULL.
 *   present_a[X]  the count marginal of X is positive; r_a the number of present states (N counts as one); likewise b.
 *   poly_out[K][C]  bit 0: r_a > 1, bit 1: r_b > 1.
 *   neff_out[C]   the fp64 of the long-double sum of the weights hdw[s] of the members in sequence order (the rule of ldw_set_weights' neff).
 *   mi_out[K][C]  the sum over the cells whose two states are present, X outer and Y inner, in fp64, of
 *                     (pxy / den) log(pxy / (pX pY + r_a r_b / 4 + r_a pX / 2 + r_b pY / 2) den),
 *                 pxy = fixed[X][Y] / 2^F + 1/2, pX = (sum over Y of fixed[X][Y]) / 2^F, pY likewise, den = neff_c + r_a r_b / 2: the reference's formula
 *                 with the intended RXY on the members alone.  Finite for every cluster with a member; where both SNPs are monomorphic in c the sum is
 *                 log 1 and 0 is returned outright.
 *   mi_all_out[K] the same over all labelled sequences (the tables summed over the clusters, neff summed over the labelled sequences in sequence order).
 * The cell order is fixed and every sum is an integer: equal inputs give equal bits whatever the chunking or the numbering of the clusters.  Pairs go in
 * chunks whose working memory stays within 1 GiB; LDW_LIN_CHUNK=k in the environment, read at every call, forces chunks of k pairs: a test hook.
 * ldw_ctx_last_timing afterwards: [0] the pairs, [1] the bit rows of the chunks' SNPs, [2] the copies out, [3] their sum.
 * Refused on the host before anything is launched, the context staying usable — LDW_ERR_STATE: no alignment or no weights resident.  LDW_ERR_ARG: K < 1;
 * C outside 1..65536; a label outside [-1, C); every label -1; a SNP index outside [0, L); a null pointer among the required ones.  The message names the
 * index. */
int ldw_links_stratified(ldw_ctx *ctx, const int32_t *pair_a, const int32_t *pair_b, int64_t K, const int32_t *labels, int32_t C, double *mi_out,
                         double *mi_all_out, uint8_t *poly_out, double *neff_out, int64_t *counts_out, int64_t *fixed_out, int *frac_bits_out);

/* ---- (19) permutation p-values for links, within lineages -------------------------------------------------------------------------------
 * ldw_links_permuted: for the SNP pairs (pair_a[i], pair_b[i]), i < K, labels[N] and C exactly as ldw_links_stratified takes them (HOST), the weighted MI
 * over all labelled sequences and its null distribution under B permutations of SNP b's states among the sequences of every cluster.  Needs the alignment
 * and the weights resident.
 *   P            the number of sequences with labels >= 0 (*p_out).  order0[P]: those sequences sorted by (label, sequence index).
 *   order_r[P]   for replicate r in [0, B): the same sequences stably sorted by the 56-bit key (label << 40) | h(seed, r, s); equal keys keep ascending
 *                sequence index.  With all arithmetic mod 2^64:
 *                    z = seed + 0x9E3779B97F4A7C15 (r + 1) + 0xD1B54A32D192ED03 (s + 1)
 *                    z = (z ^ z >> 30) 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) 0x94D049BB133111EB;  z ^= z >> 31;  h = z >> 24.
 *                A replicate is thus a permutation within every cluster and a function of (labels, seed, r) alone.
 *   fixed_r[X][Y]  the sum over p of V[order0[p]] wherever states[a][order0[p]] == X and states[b][order_r[p]] == Y (states above 4 count as 4, N);
 *                counts_r the same with 1 in place of V.  The weight stays with the sequence and with SNP a: only b's states move.
 *   mi_r         the formula of (18) on that one table over all labelled sequences: neff is mi_all's (the long-double sum of hdw over the labelled sequences
 *                in sequence order), r_a and r_b come from the count marginals, "both monomorphic" returns 0 outright.  It is evaluated by the same device
 *                function as mi_all, so equal integer tables give equal bits.
 * Outputs (HOST): mi_obs_out[K] = mi_r under the identity order (order0), bit-equal to ldw_links_stratified's mi_all_out for the same inputs; n_ge_out[K]
 * (int32) the replicates with mi_r >= mi_obs, an fp64 compare on the device's own values; null_max_out[K] the largest mi_r; and, each of which may be NULL,
 * null_out[K][B] (fp64) every mi_r, fixed_out[K][B][25] (int64) every fixed_r, order_out[B][P] (int32) every order_r; *frac_bits_out as with
 * ldw_links_stratified.  Replicates go in batches of at most 256 — one stable radix sort per batch — sized so that keys, values and sort storage stay within
 * 1 GiB; pairs go in chunks whose per-batch values and tables stay within 1 GiB.  No result depends on either: counts are integers, maxima are maxima.
 * Test hooks in the environment, read at every call: LDW_PERM_BATCH=k forces batches of k replicates (k <= 256), LDW_PERM_CHUNK=k chunks of k pairs,
 * LDW_PERM_LDS=m the kernel form m (0: weights and both state arrays in LDS, 1: the state arrays, 2: none) or the next one that fits.
 * ldw_ctx_last_timing afterwards: [0] the pair kernel (with the counts), [1] keys and sorts, [2] the copies out, [3] their sum.
 * Refused on the host before anything is launched, the context staying usable — LDW_ERR_STATE: no alignment or no weights resident.  LDW_ERR_ARG: K < 1;
 * B outside 1..2^24; C outside 1..65536; a label outside [-1, C); every label -1; a SNP index outside [0, L); a null pointer among the required ones.  The
 * message names the index.  The call takes its working memory (besides the above, 28 bytes per pair) and gives it back; the alignment, the weights, the SNP
 * metadata and the link tables stay as they are. */
int ldw_links_permuted(ldw_ctx *ctx, const int32_t *pair_a, const int32_t *pair_b, int64_t K, const int32_t *labels, int32_t C, int32_t B, uint64_t seed,
                       double *mi_obs_out, int32_t *n_ge_out, double *null_max_out, double *null_out, int64_t *fixed_out, int32_t *order_out, int64_t *p_out,
                       int *frac_bits_out);

/* ---- (20) LD decay: a histogram, circular distance bin x MI bucket, of EVERY SNP pair of a block list ------------------------------------
 * ldw_mi_profile needs the alignment, the weights and the SNP meta data, as ldw_mi_all_pairs does (LDW_ERR_STATE without them, and for a context that holds
 * positions only, ldw_set_positions).
 *   blocks[nblocks][4]  (from_s, from_e, to_s, to_e), 1-based inclusive, as make_blocks emits them (HOST).  A block is diagonal (both ranges equal) or its
 *                ranges are disjoint; any other overlap is LDW_ERR_ARG.
 *   the pairs    of a diagonal block: the local pairs a_loc > b_loc; of any other block: every (a_loc, b_loc) with a_loc != b_loc — the reference drops the
 *                local diagonal there (R/computePairwiseMI.R:306-310), and so does this.  The total is the sum of n_sr + n_lr_total of ldw_block_stats
 *                after ldw_mi_all_pairs over the same blocks.
 *   the value    of a pair: what ldw_mi_block stores at [a_loc + b_loc * nf] for the block under the same quirk_mode (quirk Q1 makes it depend on the
 *                block's geometry, which is why the blocks are an input).
 *   distance bin len = 0.5 g - |(POS[to] - POS[from]) mod g - 0.5 g|, the len column of the link tables.  cuts[n_cut] (HOST): finite, non-negative, strictly
 *                ascending, 0 <= n_cut <= 1023 (LDW_ERR_ARG otherwise).  The bin of a pair is the number of cuts strictly below len: bins are
 *                (c_(k-1), c_k], n_cut + 1 of them, and a cut equal to sr_dist separates the pass's short range (len <= sr_dist) from its long range.
 *   MI bin       mi_bucket(mi) >> mi_shift, mi_shift in 0..6, NB = 4096 >> mi_shift bins.  mi_bucket is the long-range selection's rule, taken from the IEEE
 *                bits of the value: 0 for negatives, +-0 and values below 2^-20; else ((bits >> 45) - ((1023 - 20) << 7)), at most 4095: 128 buckets per
 *                octave, lower edge of bucket B >= 1 the double with bits (B + ((1023 - 20) << 7)) << 45.
 * Outputs (HOST): hist_out[n_cut + 1][NB] counts; max_out[n_cut + 1] (may be NULL) the largest value of every distance bin, the device's own bits, NaN for
 * a bin without a pair; *npairs_out the number of pairs.  Integer adds and a maximum: nothing depends on the order of evaluation.
 * The link tables and the ldw_block_stats of an earlier pass stay as they were.  ldw_ctx_last_timing afterwards: [0] the blocks' GEMM + epilogue, [1] the
 * histogram kernels, [2] 0, [3] their sum.  The call runs on the context's stream and returns when the outputs are written. */
int ldw_mi_profile(ldw_ctx *ctx, const int32_t *blocks, int64_t nblocks, int quirk_mode, const double *cuts, int32_t n_cut, int32_t mi_shift,
                   uint64_t *hist_out, double *max_out, int64_t *npairs_out);

/* ---- (21) per-SNP MI summary over EVERY SNP pair of a block list: the background of each SNP, in two distance classes ---------------------
 * ldw_mi_snp_summary requires and refuses what ldw_mi_profile does (20): the alignment, the weights and the SNP meta data; blocks diagonal or disjoint.
 *   the pairs    exactly those of ldw_mi_profile over the same blocks, with the same values under the same quirk_mode.
 *   the class    of a pair: c = 0 (short range) if len = 0.5 g - |(POS[to] - POS[from]) mod g - 0.5 g| <= sr_dist, else c = 1 (long range): the pass's own
 *                split.  sr_dist is non-negative and not NaN (LDW_ERR_ARG otherwise); +inf makes every pair short range.
 *   contribution every pair contributes to BOTH of its SNPs, the from-SNP and the to-SNP.  Per SNP i and class c (outputs [2][L], class-major, HOST):
 *     n_out      the number of partners.
 *     sumq_out   the sum of q(mi) = llrint(mi * 2^40) over the partners: the product is an exact scaling, the rounding is to nearest, ties to even.  A value
 *                that is not finite or has |mi| >= 2^22 adds 0 and is counted (ldw_snp_summary_report).  |q| < 2^62; with MI <= ln 5 (|q| < 2^41) and at
 *                most 2^21 partners the sum stays below 2^62.  The mean MI of SNP i with its partners of class c is sumq / n / 2^40.
 *     max_out    (may be NULL) the largest value in the order of the IEEE bits (-0 below +0), the device's own bits; NaN where n == 0.
 *     nge_out    (may be NULL) the number of partners with mi >= thr[c], an fp64 comparison: +inf counts no finite value, a NaN value never counts.
 *   npairs_out[2] the pairs of each class: sum_i n[c][i] == 2 npairs[c]; npairs[0] / npairs[1] equal the sums of n_sr / n_lr_total of ldw_block_stats after
 *                ldw_mi_all_pairs with the same sr_dist over the same blocks.
 * Integer adds and a maximum: nothing depends on the order of evaluation.  The link tables and the ldw_block_stats of an earlier pass stay as they were.
 * ldw_ctx_last_timing afterwards: [0] the blocks' GEMM + epilogue, [1] the summary kernels, [2] 0, [3] their sum.  The call runs on the context's stream
 * and returns when the outputs are written. */
int ldw_mi_snp_summary(ldw_ctx *ctx, const int32_t *blocks, int64_t nblocks, int quirk_mode, double sr_dist, const double *thr, int64_t *n_out,
                       int64_t *sumq_out, double *max_out, int64_t *nge_out, int64_t *npairs_out);

/* ---- (22) selection by a corrected score over EVERY SNP pair of a block list, with each SNP's best partner ----------------------------------
 * ldw_mi_score_scan and ldw_mi_score_links require and refuse what ldw_mi_profile does (20): the alignment, the weights and the SNP meta data; blocks
 * diagonal or disjoint.  Blocks, pair set and values are exactly those of (20) and (21) under the same quirk_mode.
 *   the score    of the pair of the global SNPs (A, B): s = mi - w[A] * w[B], two IEEE fp64 operations, the product and then the difference, never one
 *                fused multiply-add (csrc/ldw_score.h states it once for the device and the host).  The product is commutative: s does not depend on which
 *                SNP is the from-SNP.  w[L] (HOST) must be finite: LDW_ERR_ARG otherwise, the message naming the index.  The average product correction is
 *                w = mean / sqrt(overall mean); the entries do not know that: any rank-one correction is a w.  A pair whose MI is NaN has a NaN score.
 *   the class mask cls_mask = 1: the pairs with len <= sr_dist (short range), 2: the pairs beyond (long range), 3: both; len, sr_dist and the class of a pair
 *                as in (21).  LDW_ERR_ARG for any other mask, for a negative or NaN sr_dist.  Pairs outside the mask take no part in anything below.
 * ldw_mi_score_scan — outputs (HOST):
 *   hist_out[4096]  hist_out[B] counts the pairs with mi_bucket(s) == B, the long-range selection's rule as (20) states it (0 for negatives, +-0 and values
 *                below 2^-20).  A NaN score is in no bucket.
 *   best_out[L]  the largest score of SNP i over its partners in the order of the IEEE bits (-0 below +0), the device's own bits; NaN where there is none.
 *                Every pair contributes to both of its SNPs; a NaN score is never a best.
 *   *npairs_out  the pairs inside the mask: the sum of hist_out plus the NaN scores of ldw_score_select_report.
 * ldw_mi_score_links — every pair inside the mask with s >= thr (an fp64 comparison: a NaN score is never listed) is listed once as a_out / b_out (the
 *   from-SNP and the to-SNP, global and 0-based), mi_out and score_out (the device's own bits), in no stated order.  *count_out is the exact number of such
 *   pairs whatever cap is; where it exceeds cap the call returns LDW_ERR_SIZE with *count_out written and the lists undefined; nothing is written past
 *   cap entries.  cap = 0 with null lists is a pure count.
 *   partner_out[L] (int32, may be NULL; needs best_in[L], LDW_ERR_ARG otherwise): the smallest global index j among i's partners inside the mask whose score
 *                has the key of best_in[i] (equal IEEE bits); -1 where best_in[i] is NaN or no partner matches.  With best_in = best_out of a scan with the
 *                same arguments it names each SNP's best partner.  A 32-bit integer minimum: nothing depends on the order of evaluation.
 * Integer adds, maxima of an ordered key and integer minima only.  The link tables and the ldw_block_stats of an earlier pass stay as they were.
 * ldw_ctx_last_timing afterwards: [0] the blocks' GEMM + epilogue, [1] the scan or links kernels, [2] 0, [3] their sum.  Both calls run on the context's
 * stream and return when the outputs are written. */
int ldw_mi_score_scan(ldw_ctx *ctx, const int32_t *blocks, int64_t nblocks, int quirk_mode, double sr_dist, int cls_mask, const double *w, uint64_t *hist_out,
                      double *best_out, int64_t *npairs_out);
int ldw_mi_score_links(ldw_ctx *ctx, const int32_t *blocks, int64_t nblocks, int quirk_mode, double sr_dist, int cls_mask, const double *w, double thr,
                       const double *best_in, int64_t cap, int32_t *a_out, int32_t *b_out, double *mi_out, double *score_out, int64_t *count_out,
                       int32_t *partner_out);

/* ---- (23) the co-change scan: the branches of a tree on which two SNPs both change, over EVERY pair of the SNPs that change often enough -----
 * parent, tip_seq, nodes and gap_mode exactly as (17) takes and refuses them; further nodes <= 2^21, which keeps the products below inside int64.
 * B = nodes - 1 is the number of branches.  changes[i] is SNP i's parsimony score (17): the popcount of its bitmap of changed branches.
 *   eligible     SNP i is eligible when changes[i] >= min_changes (min_changes >= 1).  M is their number; they are taken in ascending SNP index.
 *   the pair set P: the unordered pairs i < j of eligible SNPs; where min_len >= 0 only those with circ_len(POS[j], POS[i], g) > min_len, the len column of the
 *                link tables (0.5 g - |(POS[j] - POS[i]) mod g - 0.5 g|), closed below as the pass's sr_dist is.  min_len < 0: no distance is computed and
 *                neither SNP meta data nor positions are needed.  NaN is refused.
 *   qualifying   co = popcount(bits_i & bits_j), the branches on which both change (ldw_tree_cochanges' co_out).  A pair of P qualifies when
 *                co * B >= min_lift * changes[i] * changes[j], an int64 comparison: co is at least min_lift times what two independent branch sets would
 *                share.  min_lift is an integer in [0, 2^20]; 0 qualifies every pair of P.
 * ldw_tree_cochange_scan — outputs (HOST):
 *   changes_out[L]  the score of every SNP.
 *   hist_out[1024]  the qualifying pairs per min(co, 1023).
 *   best_out[L]  (int32) the largest co of SNP i over its qualifying partners; -1 where there are none, ineligible SNPs included.
 *   nge_out[L]   (int64) the qualifying partners of SNP i with co >= min_co (min_co >= 0).
 *   npairs_out[2]  |P| and the number of qualifying pairs; the second equals the sum of hist_out.
 *   Every pair adds to both of its SNPs.
 * ldw_tree_cochange_links — every qualifying pair with co >= min_co is listed once as a_out < b_out (global, 0-based) and co_out, in no stated order.
 *   *count_out is the exact number of such pairs whatever cap is; where it exceeds cap the call returns LDW_ERR_SIZE with *count_out written and the lists
 *   undefined; nothing is written past cap entries.  cap = 0 with null lists is a pure count: the contract of ldw_mi_score_links (22).
 *   partner_out[L] (int32, may be NULL; needs best_in[L], LDW_ERR_ARG otherwise): the smallest j among i's qualifying partners whose co == best_in[i]; -1
 *                where best_in[i] < 0, where nothing matches and for an ineligible SNP.  With best_in = best_out of a scan with the same arguments it names
 *                each SNP's best partner.
 * Integer adds, integer maxima and integer minima only: nothing depends on the order of evaluation, on the chunks of the passes (LDW_PARS_CHUNK) or on the
 * bands the pair kernel is launched in (at most 65 535 tile rows each; LDW_COSCAN_ROWS=k in the environment, read at every call, forces bands of k tile
 * rows: a test hook).  M of 0 or 1 is legal: zero pairs, best all -1.  ldw_ctx_last_timing afterwards: [0] the pair kernels, [1] the parsimony passes and
 * gathers, [2] the copies out, [3] their sum.
 * Refused on the host before anything is launched, the context staying usable — LDW_ERR_STATE: no alignment resident, or min_len >= 0 without positions
 * (ldw_set_snp_meta).  LDW_ERR_ARG: whatever (17) refuses; nodes > 2^21; min_changes < 1; min_co < 0; min_lift outside [0, 2^20]; min_len NaN; partner_out
 * without best_in; a null required pointer.  Both calls run on the context's stream, take their working memory (the scores' node sets as (17), then
 * ceil(nodes / 32) x 4 bytes per eligible SNP for the bitmaps) and give it back; the alignment, the weights, the SNP metadata and the link tables stay as
 * they are. */
int ldw_tree_cochange_scan(ldw_ctx *ctx, const int32_t *parent, const int32_t *tip_seq, int64_t nodes, int32_t gap_mode, int32_t min_changes, int32_t min_co,
                           int64_t min_lift, double min_len, int32_t *changes_out, uint64_t *hist_out, int32_t *best_out, int64_t *nge_out, int64_t *npairs_out);
int ldw_tree_cochange_links(ldw_ctx *ctx, const int32_t *parent, const int32_t *tip_seq, int64_t nodes, int32_t gap_mode, int32_t min_changes, int32_t min_co,
                            int64_t min_lift, double min_len, const int32_t *best_in, int64_t cap, int32_t *a_out, int32_t *b_out, int32_t *co_out,
                            int64_t *count_out, int32_t *partner_out);

/* ---- (24) segment x segment map over EVERY SNP pair of a block list, with each cell's best pair ----------------------------------------------
 * ldw_mi_segment_map and ldw_mi_segment_best require and refuse what ldw_mi_profile does (20): the alignment, the weights and the SNP meta data; blocks
 * diagonal or disjoint.  Blocks, pair set and per-pair values are exactly those of (20)-(22) under the same quirk_mode.
 *   segments     seg[L] (HOST) labels the SNPs: seg[i] in -1..S-1, S in 1..8192 (LDW_ERR_ARG otherwise, the message naming the first bad index).  A pair with
 *                either SNP at -1 takes part in nothing.  The ids need not be contiguous runs or ascend along the genome: equal ids far apart are one segment.
 *   class mask   sr_dist and cls_mask exactly as (22); pairs outside the mask take part in nothing.
 *   the value    of the pair of the global SNPs (A, B): v = mi when w == NULL, else v = mi - w[A] * w[B], the score of (22) (csrc/ldw_score.h); w[L] (HOST) must
 *                be finite (LDW_ERR_ARG, the message naming the index).
 *   the cell     of a pair is (min(seg[A], seg[B]), max(seg[A], seg[B])): a pair counts once, whichever SNP is the from-SNP.  Every matrix is row-major [S][S];
 *                only cells with row <= column are written, the rest stay 0 (NaN in max_out).
 * ldw_mi_segment_map — per cell (HOST):
 *   n_out        the number of pairs.
 *   nge_out      (may be NULL) the pairs with v >= thr, an fp64 comparison: a NaN value never counts, thr = +inf counts nothing.
 *   sum_lo_out, sum_hi_out  (both or neither) the sum of q(v) = llrint(v * 2^40), the product and the rounding of (21), in two words so that no cell can overflow:
 *                sum_lo = sum of (q & (2^24 - 1)), sum_hi = sum of (q >> 24) (an arithmetic shift); the exact sum is sum_hi * 2^24 + sum_lo
 *                (csrc/ldw_segmap.h).  A value that is not finite or has |v| >= 4 adds 0 to both words and is counted (ldw_segment_map_report); it still counts
 *                in n, nge and max.  With |q| <= 2^42 both words stay below 2^63 for any cell of fewer than 2^39 pairs; a block list of 2^39 pairs or more is
 *                LDW_ERR_SIZE.  The mean value of a cell is (sum_hi * 2^24 + sum_lo) / n / 2^40.
 *   max_out      (may be NULL) the largest value in the order of the IEEE bits (-0 below +0), the device's own bits; NaN where n == 0.  A NaN value is never a
 *                maximum (a cell of NaN values only has NaN).
 *   *npairs_out  the pairs inside the mask with both segments >= 0: the sum of n_out.
 * ldw_mi_segment_best — pair_out[S * S] (uint64): per cell the smallest ((uint64)min(A, B) << 32) | max(A, B) over the cell's pairs inside the mask whose value
 *   has the key of max_in[cell] (equal IEEE bits); all-ones where max_in[cell] is NaN or nothing matches.  With max_in = max_out of a map call with the same
 *   arguments it names the pair behind each maximum.  A 64-bit integer minimum.
 * Integer adds, maxima of an ordered key and integer minima only: nothing depends on the order of evaluation, and there is no floating-point atomic.  Device
 * memory: 40 S^2 bytes for the map (16 S^2 for the best pairs) plus the per-SNP vectors, one working buffer that the call takes and gives back.  The link
 * tables and the ldw_block_stats of an earlier pass stay as they were.  ldw_ctx_last_timing afterwards: [0] the blocks' GEMM + epilogue, [1] this entry's
 * kernels, [2] 0, [3] their sum.  Both calls run on the context's stream and return when the outputs are written. */
int ldw_mi_segment_map(ldw_ctx *ctx, const int32_t *blocks, int64_t nblocks, int quirk_mode, const int32_t *seg, int32_t S, double sr_dist, int cls_mask,
                       const double *w, double thr, int64_t *n_out, int64_t *nge_out, int64_t *sum_lo_out, int64_t *sum_hi_out, double *max_out,
                       int64_t *npairs_out);
int ldw_mi_segment_best(ldw_ctx *ctx, const int32_t *blocks, int64_t nblocks, int quirk_mode, const int32_t *seg, int32_t S, double sr_dist, int cls_mask,
                        const double *w, const double *max_in, uint64_t *pair_out);

/* ---- small native helpers kept for finest-grain A/B parity (host memory) -------------------- */
/* .compareToRow src/computeMI.cpp:25-41: ret[j] = any(x[j,] in y); x is nr x nc column-major */
int ldw_compare_to_row(const double *x, int64_t nr, int64_t nc, const double *y, int64_t ny, uint8_t *ret);
/* .vecPosMatch src/computeMI.cpp:44-59: 1-based first position of x[i] in y, 0 if absent */
int ldw_vec_pos_match(const double *x, int64_t nx, const double *y, int64_t ny, double *ret);
/* .compareTriplet src/computeMI.cpp:63-77 */
int ldw_compare_triplet(const double *MI0X, const double *MI0Z, int64_t n, double MI0, int *ret);
/* .fast_intersect src/fintersect.cpp:6-32; out capacity >= min(na, nb); *n_out = result length */
int ldw_fast_intersect(const int32_t *A, int64_t na, const int32_t *B, int64_t nb, int32_t *out,
                       int64_t *n_out);

#ifdef __cplusplus
}
#endif
#endif /* LDWEAVER_AMD_H */
