// The search of annotated link files on the device (include/ldweaver_amd.h 14): grep(gene, pos1_ann / pos2_ann) of
// create_network_for_gene (R/createNetworkPlot.R:180, :196, :244, :259) over sr_links_annotated.tsv / lr_links_annotated.tsv, with literal needles.
// The file goes through the reader's chunk pass (TsvPass: the feeder, the pinned double buffer and its '\n' padding, k_tsv_count / k_tsv_starts: ldw_links_read.h);
// k_links_grep then gives every row to one wave: the lanes find the row's tabs by ballots, five of them parse the numeric cells (ldw_tsv_cell.h), all of
// them walk the text positions of the two annotation fields against the needles, bucketed by first byte in LDS, and a kept row is appended by one atomic.
// The host queues a chunk's search, reads the next chunk meanwhile, then sorts the few kept rows of the chunk back into file order and cuts their three
// strings from the pinned text it still holds.
//
// Bounds: a row's bytes are read from its first byte to its '\n' (a position at or past the chunk's `cut` bytes is not read: it counts as '\n'), the
// numeric cells by parse_cell (at most three bytes past a byte that is no separator: the '\n' tail of TSV_TAIL), a needle only where it fits inside its
// field.  A kept row is written only where its slot lies below the record arrays' capacity.
#pragma clang fp contract(off)
#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "ldw_work.h"
#include "ldw_dev.h"
#include "ldw_fasta.h"
#include "ldw_links_read.h"
#include "ldw_tsv_cell.h"

using namespace ldw;

namespace {

constexpr int GREP_BLOCK = 256, GREP_WAVES = GREP_BLOCK / 64;
constexpr int GREP_MAX_NEEDLES = 1024, GREP_MAX_WORDS = GREP_MAX_NEEDLES / 64, GREP_MAX_LEN = 255;
constexpr uint32_t GREP_FIRST_RECORDS = 16384;   // records a chunk gets room for at first; a chunk that keeps more rows is searched again with room for all
constexpr int GREP_NUM = 5, GREP_STR = 3;   // pos1 pos2 len ARACNE MI; pos1_ann pos2_ann links

struct GrepResult {   // what a chunk's kernel reports
    unsigned long long bad;   // min over the refused rows of row << 16 | column (1-based) << 8 | reason; ~0: none
    uint32_t kept, pad;
};

struct GrepRec {   // one kept row
    double num[GREP_NUM];
    uint32_t row;                 // in the chunk (the header line counts where the chunk holds it)
    uint32_t slow;                // bit k: num[k] is left to the host's strtod
    uint32_t num_at[GREP_NUM];    // first byte of the numeric cells, from the chunk's first byte
    uint32_t str_at[GREP_STR], str_len[GREP_STR];
    uint32_t pad;
};
static_assert(sizeof(GrepRec) == 96, "GrepRec is copied as bytes");

struct GrepParams {
    int ncols, n_needles, nw, drop_sy, drop_ind;
    uint32_t skip;                            // rows of the chunk before the first data row (1: the chunk holds the header)
    int col_num[GREP_NUM], col_str[GREP_STR];   // 0-based file columns
};

struct NeedleTables {   // needles sorted by first byte: bucket b = [bstart[b], bstart[b + 1])
    const uint16_t *bstart;   // [257]
    const uint32_t *off;      // [n] first byte in blob
    const uint16_t *orig;     // [n] the caller's index
    const uint8_t *len;       // [n]
    const uint8_t *blob;
};

__global__ __launch_bounds__(GREP_BLOCK) void k_links_grep(const uint8_t *__restrict__ buf, uint32_t n, const uint32_t *__restrict__ starts, uint32_t nrows,
                                                           const GrepParams P, const NeedleTables T, GrepResult *__restrict__ res, GrepRec *__restrict__ rec,
                                                           unsigned long long *__restrict__ masks, uint32_t cap) {
    __shared__ uint32_t n_off[GREP_MAX_NEEDLES];
    __shared__ uint16_t n_orig[GREP_MAX_NEEDLES];
    __shared__ uint16_t bstart[258];
    __shared__ uint8_t n_len[GREP_MAX_NEEDLES];
    __shared__ uint32_t fs[GREP_WAVES][TSV_MAX_COLS + 2];   // fs[k] = first byte of field k; field k ends before fs[k + 1] - 1
    __shared__ unsigned long long wmask[GREP_WAVES][GREP_MAX_WORDS];
    for (int k = threadIdx.x; k < P.n_needles; k += GREP_BLOCK) {
        n_off[k] = T.off[k];
        n_orig[k] = T.orig[k];
        n_len[k] = T.len[k];
    }
    for (int k = threadIdx.x; k < 257; k += GREP_BLOCK) bstart[k] = T.bstart[k];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *f = fs[wave];
    unsigned long long *wm = wmask[wave];
    for (uint32_t r = P.skip + blockIdx.x * GREP_WAVES + wave; r < nrows; r += gridDim.x * GREP_WAVES) {
        const uint32_t s = starts[r];
        // the row's tabs and its end
        uint32_t nf = 1, e = s;
        if (lane == 0) f[0] = s;
        for (uint32_t base = s;; base += 64) {
            const uint32_t pos = base + lane;
            const uint8_t ch = pos < n ? buf[pos] : (uint8_t)'\n';
            const unsigned long long nl = __ballot(ch == '\n');
            unsigned long long tabs = __ballot(ch == '\t');
            if (nl) {
                const int j = __ffsll((long long)nl) - 1;
                tabs &= (1ull << j) - 1ull;
                e = base + (uint32_t)j;
            }
            while (tabs) {
                const int k = __ffsll((long long)tabs) - 1;
                tabs &= tabs - 1;
                if (nf <= (uint32_t)P.ncols && lane == 0) f[nf] = base + (uint32_t)k + 1;
                ++nf;
            }
            if (nl) break;
        }
        const uint32_t e_trim = (e > s && buf[e - 1] == '\r') ? e - 1 : e;
        if (nf <= (uint32_t)P.ncols && lane == 0) f[nf] = e_trim + 1;
        if (lane < P.nw) wm[lane] = 0ull;
        __threadfence_block();   // (the wave's lanes read what lane 0 wrote)
        const uint32_t have = min(nf, (uint32_t)P.ncols);   // fields with both ends in f[]
        // faults, the leftmost first
        uint32_t bad = ~0u;
        double v = 0.0;
        bool slow = false;
        uint32_t cell_at = 0;
        if (e - s > (uint32_t)TSV_LINE_MAX) {
            bad = 1u << 8 | BAD_LONG;
        } else {
            if (nf < (uint32_t)P.ncols) bad = (nf + 1) << 8 | BAD_MISSING;
            if (nf > (uint32_t)P.ncols) bad = (uint32_t)(P.ncols + 1) << 8 | BAD_EXTRA;
            if (lane < GREP_NUM) {
                const uint32_t col = (uint32_t)P.col_num[lane];
                if (col < have) {
                    cell_at = f[col];
                    const uint32_t cell_len = f[col + 1] - 1 - cell_at;
                    uint32_t i = 0;
                    bool plain;
                    const int kind = parse_cell(buf + cell_at, i, v, plain);
                    slow = kind == CELL_SLOW;
                    bool ok = kind != CELL_BAD && i == cell_len;
                    if (!ok && lane == 3) {   // ARACNE as R's write.table writes a logical column (lr_links_annotated.tsv): TRUE / FALSE
                        const uint8_t *q = buf + cell_at;
                        if (cell_len == 4 && q[0] == 'T' && q[1] == 'R' && q[2] == 'U' && q[3] == 'E') {
                            v = 1.0;
                            ok = true;
                        } else if (cell_len == 5 && q[0] == 'F' && q[1] == 'A' && q[2] == 'L' && q[3] == 'S' && q[4] == 'E') {
                            v = 0.0;
                            ok = true;
                        }
                        slow = slow && !ok;
                    }
                    if (!ok) bad = min(bad, (col + 1) << 8 | BAD_CELL);
                }
            }
            for (int o = 32; o > 0; o >>= 1) bad = min(bad, (uint32_t)__shfl_xor((int)bad, o, 64));
        }
        if (bad != ~0u) {
            if (lane == 0) atomicMin(&res->bad, (unsigned long long)r << 16 | bad);
            continue;
        }
        // the needles inside pos1_ann and pos2_ann
        const uint32_t a0 = f[P.col_str[0]], a1 = f[P.col_str[0] + 1] - 1, b0 = f[P.col_str[1]], b1 = f[P.col_str[1] + 1] - 1;
        const uint32_t la = a1 - a0, total = la + (b1 - b0);
        for (uint32_t t = lane; t < total; t += 64) {
            const uint32_t pos = t < la ? a0 + t : b0 + (t - la), fend = t < la ? a1 : b1;
            const uint8_t ch = buf[pos];
            for (uint32_t j = bstart[ch]; j < bstart[ch + 1]; ++j) {
                const uint32_t len = n_len[j];
                if (pos + len > fend) continue;
                const uint8_t *nd = T.blob + n_off[j];
                uint32_t k = 1;
                while (k < len && nd[k] == buf[pos + k]) ++k;
                if (k == len) atomicOr(&wm[n_orig[j] >> 6], 1ull << (n_orig[j] & 63));
            }
        }
        __threadfence_block();
        const unsigned long long word = lane < P.nw ? wm[lane] : 0ull;
        bool keep = __ballot(word != 0ull) != 0ull;
        const uint32_t l0 = f[P.col_str[2]], l1 = f[P.col_str[2] + 1] - 1;
        if (keep && P.drop_sy && l1 - l0 == 5)
            keep = !(buf[l0] == 's' && buf[l0 + 1] == 'y' && buf[l0 + 2] == 'X' && buf[l0 + 3] == 's' && buf[l0 + 4] == 'y');
        const double aracne = __shfl(v, 3, 64);
        const unsigned long long slow_mask = __ballot(slow);   // (lanes 0..4)
        if (keep && P.drop_ind && !(slow_mask >> 3 & 1) && !(aracne == 1.0)) keep = false;   // (a slow ARACNE cell: the host decides)
        if (keep) {
            uint32_t slot = 0;
            if (lane == 0) slot = atomicAdd(&res->kept, 1u);
            slot = (uint32_t)__shfl((int)slot, 0, 64);
            if (slot < cap) {
                GrepRec *o = rec + slot;
                if (lane < GREP_NUM) {
                    o->num[lane] = v;
                    o->num_at[lane] = cell_at;
                }
                if (lane < GREP_STR) {
                    const uint32_t at = f[P.col_str[lane]];
                    o->str_at[lane] = at;
                    o->str_len[lane] = f[P.col_str[lane] + 1] - 1 - at;
                }
                if (lane == 0) {
                    o->row = r;
                    o->slow = (uint32_t)slow_mask;
                    o->pad = 0;
                }
                if (lane < P.nw) masks[(size_t)slot * P.nw + lane] = word;
            }
        }
        __threadfence_block();   // (the next row's writes to f[] and wm[] come after this row's reads)
    }
}

__global__ void k_grep_init(GrepResult *res) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        res->bad = ~0ull;
        res->kept = 0;
        res->pad = 0;
    }
}

struct GrepState {
    DevBuf tables, work;                 // the needle tables and the result word; a chunk's records and mask words
    PinnedBuf pin_res;                   // GrepResult: pinned twin of the result word
    Event ev[2];                         // before k_tsv_starts, after the search kernel
    // the last result (host)
    int nw = 0;
    std::vector<int64_t> row;
    std::vector<double> num;             // [kept][5]
    std::vector<uint64_t> mask;          // [kept][nw]
    std::vector<uint8_t> text;
    std::vector<int64_t> text_off;       // [3 kept + 1]
    int64_t data_rows = 0;
    double ms[8] = {};                   // total, read (host), copy, line kernels, search kernel, chunks, bytes, kept rows
    bool valid = false;
};

GrepState *grep_state(ldw_ctx *c) {
    if (!c->grep) c->grep = new GrepState();
    return static_cast<GrepState *>(c->grep);
}

const char *const GREP_NAMES[GREP_NUM + GREP_STR] = {"pos1", "pos2", "len", "ARACNE", "MI", "pos1_ann", "pos2_ann", "links"};

}  // namespace

namespace ldw {
void grep_release(ldw_ctx *c) { release_state<GrepState>(c, c->grep); }

int64_t grep_trim(ldw_ctx *c) {
    auto *g = static_cast<GrepState *>(c->grep);
    if (!g) return 0;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    const int64_t n = (int64_t)(g->work.cap + g->row.capacity() * 8 + g->num.capacity() * 8 + g->mask.capacity() * 8 + g->text.capacity() + g->text_off.capacity() * 8);
    g->work.release();
    g->valid = false;
    std::vector<int64_t>().swap(g->row);
    std::vector<double>().swap(g->num);
    std::vector<uint64_t>().swap(g->mask);
    std::vector<uint8_t>().swap(g->text);
    std::vector<int64_t>().swap(g->text_off);
    return n;
}
}  // namespace ldw

extern "C" {

int ldw_links_grep(ldw_ctx *c, const char *path, const uint8_t *needles, const int32_t *needle_off, int32_t n_needles, int32_t flags, int64_t chunk_bytes,
                   int64_t *rows_out, int64_t *text_bytes_out, int64_t *data_rows_out) {
    if (rows_out) *rows_out = 0;
    if (text_bytes_out) *text_bytes_out = 0;
    if (data_rows_out) *data_rows_out = 0;
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(path != nullptr, LDW_ERR_ARG, "ldw_links_grep: null path");
    LDW_REQUIRE(n_needles >= 1 && n_needles <= GREP_MAX_NEEDLES, LDW_ERR_ARG, "ldw_links_grep: %d needles outside 1..%d", (int)n_needles, GREP_MAX_NEEDLES);
    LDW_REQUIRE(needles != nullptr && needle_off != nullptr, LDW_ERR_ARG, "ldw_links_grep: null needles");
    LDW_REQUIRE(needle_off[0] == 0, LDW_ERR_ARG, "ldw_links_grep: the needle offsets must start at 0");
    for (int j = 0; j < n_needles; ++j) {
        const int64_t len = (int64_t)needle_off[j + 1] - needle_off[j];
        LDW_REQUIRE(len >= 1 && len <= GREP_MAX_LEN, LDW_ERR_ARG, "ldw_links_grep: needle %d has %lld bytes, outside 1..%d", j, (long long)len, GREP_MAX_LEN);
    }
    LDW_REQUIRE((flags & ~(LDW_GREP_DROP_SYXSY | LDW_GREP_DROP_INDIRECT)) == 0, LDW_ERR_ARG, "ldw_links_grep: unknown flags %d", (int)flags);
    std::vector<GrepRec> recs;   // (in front of the pass: it waits for the stream before they go)
    std::vector<unsigned long long> rmask;
    std::vector<uint32_t> idx;
    TsvPass pass("ldw_links_grep", path);
    if (int rc = pass.open(chunk_bytes)) return rc;
    GrepState *g = grep_state(c);
    g->valid = false;
    g->row.clear();
    g->num.clear();
    g->mask.clear();
    g->text.clear();
    g->text_off.assign(1, 0);
    g->data_rows = 0;
    memset(g->ms, 0, sizeof(g->ms));
    const int nw = (n_needles + 63) / 64;
    g->nw = nw;
    const auto t_begin = std::chrono::steady_clock::now();
    for (auto &e : g->ev) LDW_HIP(e.ensure());
    if (int rc = g->pin_res.reserve(sizeof(GrepResult), "ldw_links_grep")) return rc;

    // the needles by first byte (a stable order inside a bucket: the caller's)
    const int32_t blob_bytes = needle_off[n_needles];
    std::vector<uint16_t> order((size_t)n_needles), h_bstart(257, 0);
    for (int j = 0; j < n_needles; ++j) order[(size_t)j] = (uint16_t)j;
    std::stable_sort(order.begin(), order.end(), [&](uint16_t a, uint16_t b) { return needles[needle_off[a]] < needles[needle_off[b]]; });
    std::vector<uint32_t> h_off((size_t)n_needles);
    std::vector<uint8_t> h_len((size_t)n_needles);
    for (int k = 0; k < n_needles; ++k) {
        const int j = order[(size_t)k];
        h_off[(size_t)k] = (uint32_t)needle_off[j];
        h_len[(size_t)k] = (uint8_t)(needle_off[j + 1] - needle_off[j]);
        ++h_bstart[(size_t)needles[needle_off[j]] + 1];
    }
    for (int b = 0; b < 256; ++b) h_bstart[(size_t)b + 1] = (uint16_t)(h_bstart[(size_t)b + 1] + h_bstart[(size_t)b]);
    Carve tv;
    auto d_res = tv.take<GrepResult>(1);
    auto d_bstart = tv.take<uint16_t>(257);
    auto d_noff = tv.take<uint32_t>(n_needles);
    auto d_orig = tv.take<uint16_t>(n_needles);
    auto d_nlen = tv.take<uint8_t>(n_needles);
    auto d_blob = tv.take<uint8_t>(blob_bytes);
    if (int rc = tv.reserve(g->tables)) return rc;
    LDW_HIP(hipMemcpyAsync(d_bstart, h_bstart.data(), 257 * 2, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(d_noff, h_off.data(), (size_t)n_needles * 4, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(d_orig, order.data(), (size_t)n_needles * 2, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(d_nlen, h_len.data(), (size_t)n_needles, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipMemcpyAsync(d_blob, needles, (size_t)blob_bytes, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));   // (the host vectors may go)
    const NeedleTables T{d_bstart, d_noff, d_orig, d_nlen, d_blob};

    if (int rc = pass.attach(c)) return rc;
    const uint8_t *d_buf = pass.d_text();

    GrepParams P;
    memset(&P, 0, sizeof(P));
    P.n_needles = n_needles;
    P.nw = nw;
    P.drop_sy = (flags & LDW_GREP_DROP_SYXSY) != 0;
    P.drop_ind = (flags & LDW_GREP_DROP_INDIRECT) != 0;
    bool have_header = false;
    int64_t lines_before_header = 0;   // empty physical lines in front of the header
    int64_t rows_seen = 0;             // non-empty lines of the chunks done (the header among them)
    int rc = LDW_OK;
    int64_t bad_row = -1;
    uint32_t bad_col = 0, bad_reason = 0;

    Carve cv;   // a chunk's records and mask words
    Carve::Slot<GrepRec> d_rec{};
    Carve::Slot<unsigned long long> d_masks{};
    uint32_t rec_cap = 0;
    bool searched = false;
    const uint32_t *d_starts = nullptr;
    // a chunk's search, queued and not waited for
    auto search = [&](int64_t cut, uint32_t skip, uint32_t nrows, uint32_t want) -> int {
        rec_cap = std::min(nrows, want);
        cv = Carve();
        d_rec = cv.take<GrepRec>(rec_cap);
        d_masks = cv.take<unsigned long long>((int64_t)rec_cap * nw);
        if (int rc2 = cv.reserve(g->work)) return rc2;
        P.skip = skip;
        LDW_LAUNCH(k_grep_init, dim3(1), dim3(64), 0, c->stream, (GrepResult *)d_res);
        const uint32_t blocks = std::min<uint32_t>((nrows - skip + GREP_WAVES - 1) / GREP_WAVES, 8192);
        LDW_LAUNCH(k_links_grep, dim3(blocks), dim3(GREP_BLOCK), 0, c->stream, d_buf, (uint32_t)cut, d_starts, nrows, P, T, (GrepResult *)d_res, (GrepRec *)d_rec,
                   (unsigned long long *)d_masks, rec_cap);
        LDW_HIP(hipMemcpyAsync(g->pin_res, d_res, sizeof(GrepResult), hipMemcpyDeviceToHost, c->stream));
        return LDW_OK;
    };
    // the rows' count known: their starts and the first search
    auto queue = [&](int64_t cut, uint32_t skip, uint32_t nrows) -> int {
        searched = have_header && nrows > skip;
        if (!searched) return LDW_OK;
        LDW_HIP(hipEventRecord(g->ev[0], c->stream));   // (behind the wait for the count: the queue has been idle since)
        if (int rc2 = pass.starts(nrows, &d_starts)) return rc2;
        if (int rc2 = search(cut, skip, nrows, GREP_FIRST_RECORDS)) return rc2;
        LDW_HIP(hipEventRecord(g->ev[1], c->stream));
        return LDW_OK;
    };
    // waits for a chunk's search; its kept rows, in file order, join the result: slow cells and strings come from the pinned text `data`
    auto finish = [&](const char *data, int64_t cut, uint32_t skip, uint32_t nrows) -> int {
        float fms = 0;
        if (searched) {
            LDW_HIP(hipEventSynchronize(g->ev[1]));
            if (hipEventElapsedTime(&fms, g->ev[0], g->ev[1]) == hipSuccess) g->ms[4] += fms;
            GrepResult r = *g->pin_res.as<GrepResult>();
            if (r.bad == ~0ull && r.kept > rec_cap) {   // more rows kept than the first guess holds: once more with room for every row
                LDW_HIP(hipEventRecord(g->ev[0], c->stream));
                if (int rc2 = search(cut, skip, nrows, nrows)) return rc2;
                LDW_HIP(hipEventRecord(g->ev[1], c->stream));
                LDW_HIP(hipEventSynchronize(g->ev[1]));
                if (hipEventElapsedTime(&fms, g->ev[0], g->ev[1]) == hipSuccess) g->ms[4] += fms;
                r = *g->pin_res.as<GrepResult>();
            }
            if (r.bad != ~0ull) {
                bad_row = rows_seen + (int64_t)(r.bad >> 16);
                bad_col = (uint32_t)(r.bad >> 8) & 0xff;
                bad_reason = (uint32_t)r.bad & 0xff;
                return LDW_ERR_ARG;
            }
            const uint32_t kept = std::min(r.kept, rec_cap);
            if (kept > 0) {
                recs.resize(kept);
                rmask.resize((size_t)kept * nw);
                LDW_HIP(hipMemcpyAsync(recs.data(), d_rec, (size_t)kept * sizeof(GrepRec), hipMemcpyDeviceToHost, c->stream));
                LDW_HIP(hipMemcpyAsync(rmask.data(), d_masks, (size_t)kept * nw * 8, hipMemcpyDeviceToHost, c->stream));
                LDW_HIP(hipStreamSynchronize(c->stream));
                idx.resize(kept);
                for (uint32_t i = 0; i < kept; ++i) idx[i] = i;
                std::sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return recs[x].row < recs[y].row; });   // file order
                for (uint32_t i = 0; i < kept; ++i) {
                    GrepRec &q = recs[idx[i]];
                    for (int m = 0; m < GREP_NUM; ++m)
                        if (q.slow >> m & 1) q.num[m] = tsv_strtod(data + q.num_at[m]);
                    if (P.drop_ind && (q.slow >> 3 & 1) && !(q.num[3] == 1.0)) continue;
                    g->row.push_back(rows_seen + (int64_t)q.row - 1);   // (the header is row 0 of the non-empty lines)
                    g->num.insert(g->num.end(), q.num, q.num + GREP_NUM);
                    g->mask.insert(g->mask.end(), rmask.begin() + (size_t)idx[i] * nw, rmask.begin() + (size_t)(idx[i] + 1) * nw);
                    for (int m = 0; m < GREP_STR; ++m) {
                        g->text.insert(g->text.end(), reinterpret_cast<const uint8_t *>(data) + q.str_at[m], reinterpret_cast<const uint8_t *>(data) + q.str_at[m] + q.str_len[m]);
                        g->text_off.push_back((int64_t)g->text.size());
                    }
                }
            }
        }
        rows_seen += nrows;
        return LDW_OK;
    };

    for (; rc == LDW_OK && pass.more(); pass.advance()) {
        const char *data = pass.begin();
        const int64_t cut = pass.cut();
        uint32_t skip = 0;
        if (!have_header) {   // the first non-empty line of the file
            int64_t at = 0;
            while (at < cut) {
                const char *nl = static_cast<const char *>(memchr(data + at, '\n', (size_t)(cut - at)));
                const int64_t len = (int64_t)(nl - (data + at));
                if (len == 0 || (len == 1 && data[at] == '\r')) {
                    ++lines_before_header;
                    at += len + 1;
                    continue;
                }
                int32_t col[GREP_NUM + GREP_STR], ncols = 0;
                if ((rc = tsv_header_columns(path, lines_before_header + 1, data + at, len, GREP_NAMES, GREP_NUM + GREP_STR, TSV_MAX_COLS, col, &ncols))) break;
                P.ncols = ncols;
                for (int q = 0; q < GREP_NUM; ++q) P.col_num[q] = col[q];
                for (int q = 0; q < GREP_STR; ++q) P.col_str[q] = col[GREP_NUM + q];
                have_header = true;
                skip = 1;
                break;
            }
            if (rc != LDW_OK) break;
        }
        // the copy and the two short line kernels are waited for: the search needs the rows' count; the next chunk is read while it runs
        uint32_t nrows = 0;
        if ((rc = pass.queue())) break;
        if ((rc = pass.wait(&nrows))) break;
        if ((rc = queue(cut, skip, nrows))) break;
        pass.prefetch();
        rc = finish(data, cut, skip, nrows);
    }
    if (rc == LDW_OK) rc = pass.feeder_refusal();   // the feeder's own refusal comes after every row before it
    if (bad_row >= 0) rc = pass.refuse_row(bad_row, bad_col, bad_reason, P.ncols);
    if (rc == LDW_OK && !have_header) {
        set_error("ldw_links_grep: %s: line 1, column 1: the file holds no header line", path);
        rc = LDW_ERR_ARG;
    }
    if (rc != LDW_OK) {
        g->row.clear();
        g->num.clear();
        g->mask.clear();
        g->text.clear();
        g->text_off.assign(1, 0);
        return rc;
    }
    g->data_rows = rows_seen - 1;
    g->valid = true;
    g->ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    g->ms[1] = pass.read_ms();
    g->ms[2] = pass.copy_ms;
    g->ms[3] = pass.line_ms;
    g->ms[5] = (double)pass.nchunks;
    g->ms[6] = (double)pass.consumed;
    g->ms[7] = (double)g->row.size();
    if (rows_out) *rows_out = (int64_t)g->row.size();
    if (text_bytes_out) *text_bytes_out = (int64_t)g->text.size();
    if (data_rows_out) *data_rows_out = g->data_rows;
    return LDW_OK;
}

int ldw_links_grep_fetch(ldw_ctx *c, int64_t capacity, int64_t text_capacity, int64_t *row_out, double *num_out, uint64_t *mask_out, uint8_t *text_out,
                         int64_t *text_off_out) {
    LDW_REQUIRE(c != nullptr, LDW_ERR_ARG, "ldw_links_grep_fetch: null context");
    auto *g = static_cast<GrepState *>(c->grep);
    LDW_REQUIRE(g && g->valid, LDW_ERR_STATE, "ldw_links_grep_fetch: no search result (ldw_links_grep)");
    const int64_t n = (int64_t)g->row.size();
    LDW_REQUIRE(capacity >= n, LDW_ERR_SIZE, "ldw_links_grep_fetch: capacity %lld < %lld rows", (long long)capacity, (long long)n);
    LDW_REQUIRE(text_capacity >= (int64_t)g->text.size(), LDW_ERR_SIZE, "ldw_links_grep_fetch: text capacity %lld < %lld bytes", (long long)text_capacity, (long long)g->text.size());
    LDW_REQUIRE(text_off_out != nullptr, LDW_ERR_ARG, "ldw_links_grep_fetch: null text offsets");
    LDW_REQUIRE(n == 0 || (row_out && num_out && mask_out), LDW_ERR_ARG, "ldw_links_grep_fetch: null output");
    LDW_REQUIRE(g->text.empty() || text_out, LDW_ERR_ARG, "ldw_links_grep_fetch: null text output");
    if (n > 0) {
        memcpy(row_out, g->row.data(), (size_t)n * 8);
        memcpy(num_out, g->num.data(), (size_t)n * GREP_NUM * 8);
        memcpy(mask_out, g->mask.data(), (size_t)n * g->nw * 8);
    }
    if (!g->text.empty()) memcpy(text_out, g->text.data(), g->text.size());
    memcpy(text_off_out, g->text_off.data(), g->text_off.size() * 8);
    return LDW_OK;
}

// ---- include/ldweaver_amd_debug.h ---------------------------------------------------------------------------------------------------------------

int ldw_links_grep_stats(ldw_ctx *c, double *out8) {
    LDW_REQUIRE(c && out8, LDW_ERR_ARG, "ldw_links_grep_stats: null argument");
    auto *g = static_cast<GrepState *>(c->grep);
    for (int k = 0; k < 8; ++k) out8[k] = g ? g->ms[k] : 0.0;
    return LDW_OK;
}

}  // extern "C"
