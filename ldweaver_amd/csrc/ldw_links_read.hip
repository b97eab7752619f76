// The native reader of numeric link tables on the device (include/ldweaver_amd.h 13): a chunk of the file's bytes goes to the device
// through one of two pinned buffers; k_tsv_count / k_tsv_starts find the first byte of every non-empty line, k_tsv_parse turns every row into doubles
// (Clinger's fast path: a decimal mantissa of at most 2^53 times or over an exact power of ten is ONE correctly rounded fp64 operation; every other
// cell goes to a list the host converts with strtod), and ldw_links_load maps a parsed table's positions to SNP indices and installs it as the
// context's short-range or long-range table.
// No contraction in this file: m * 1e^k must be rounded once, as a product.
#pragma clang fp contract(off)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "ldw_work.h"
#include "ldw_dev.h"
#include "ldw_fasta.h"
#include "ldw_links_read.h"
#include "ldw_tsv_cell.h"

using namespace ldw;

namespace {

constexpr int TSV_BLOCK = 256;
constexpr int TSV_TILE = TSV_BLOCK * 16;   // bytes of a chunk one block of the line kernels scans: 16 per thread, one 128-bit load
constexpr int TSV_STAGE = 32768;           // bytes of LDS a block of the staged parse kernel may fill with its rows' text
// reasons ldw_links_load refuses a position
enum { POS_FRACTION = 1, POS_RANGE = 2, POS_UNKNOWN = 3 };

struct TsvResult {   // what a chunk's kernels report (device, copied to a pinned twin)
    unsigned long long bad;      // min over the refused rows of row << 16 | column (1-based) << 8 | reason; ~0: none
    uint32_t rows, slow, not_int, pad;
};

// bit j: byte base + j is the first byte of a non-empty line (the byte before it is '\n', it is neither '\n' nor the '\r' of a "\r\n").  buf[-1] and
// the bytes behind the data are '\n' (TSV_FRONT, TSV_TAIL).
__device__ __forceinline__ uint32_t start_mask16(const uint8_t *__restrict__ buf, uint32_t base) {
    const uint4 w = *reinterpret_cast<const uint4 *>(buf + base);
    const uint32_t v[4] = {w.x, w.y, w.z, w.w};
    uint8_t prev = buf[(int64_t)base - 1];
    const uint8_t after = buf[base + 16];
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint8_t cur = (uint8_t)(v[j >> 2] >> (8 * (j & 3)));
        const uint8_t next = j < 15 ? (uint8_t)(v[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) : after;
        if (prev == '\n' && cur != '\n' && !(cur == '\r' && next == '\n')) m |= 1u << j;
        prev = cur;
    }
    return m;
}

__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t *sh) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

// cnt[block] = rows that start in the block's TSV_TILE bytes
__global__ __launch_bounds__(TSV_BLOCK) void k_tsv_count(const uint8_t *__restrict__ buf, uint32_t n, uint32_t *__restrict__ cnt) {
    __shared__ uint32_t sh[4];
    const uint32_t base = blockIdx.x * TSV_TILE + threadIdx.x * 16;
    const uint32_t c = base < n ? __popc(start_mask16(buf, base)) : 0;
    const uint32_t s = block_sum(c, sh);
    if (threadIdx.x == 0) cnt[blockIdx.x] = s;
}

// starts[off[block] + k] = byte offset of the block's k-th row, in file order
__global__ __launch_bounds__(TSV_BLOCK) void k_tsv_starts(const uint8_t *__restrict__ buf, uint32_t n, const uint32_t *__restrict__ off, uint32_t *__restrict__ starts) {
    __shared__ uint32_t wsum[4];
    const uint32_t base = blockIdx.x * TSV_TILE + threadIdx.x * 16;
    uint32_t m = base < n ? start_mask16(buf, base) : 0;
    const uint32_t c = __popc(m);
    // exclusive prefix of c over the block: inside the wave by shuffles, over the four waves through LDS
    uint32_t incl = c;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = off[blockIdx.x] + incl - c;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    while (m) {
        const int j = __ffs(m) - 1;
        m &= m - 1;
        starts[before++] = base + (uint32_t)j;
    }
}

// One row: ncols cells from p[0 ..] into cols[c * stride + row].  Returns 0, or column << 8 | reason of the first thing that is wrong, left to right.
// *not_int gets a bit for every column whose cell is not a plain integer literal [+-]?[0-9]+; a cell outside the fast path is appended to slow[].
template <class P>
__device__ __forceinline__ uint32_t parse_row(P p, int ncols, uint8_t sep, double *__restrict__ cols, int64_t stride, int64_t row, uint32_t row_in_chunk,
                                              uint32_t row_off, uint32_t *__restrict__ slow_n, uint2 *__restrict__ slow, uint32_t *not_int) {
    uint32_t i = 0;
    for (int col = 0; col < ncols; ++col) {
        const uint32_t cell = i;
        double v;
        bool plain;
        const int kind = parse_cell(p, i, v, plain);
        if (kind == CELL_BAD) return (uint32_t)(col + 1) << 8 | BAD_CELL;
        if (kind == CELL_SLOW) {
            const uint32_t k = atomicAdd(slow_n, 1u);
            slow[k] = make_uint2(row_in_chunk * (uint32_t)ncols + (uint32_t)col, row_off + cell);
        }
        const uint8_t c = p[i];
        if (!plain) *not_int |= 1u << col;
        const bool eol = c == '\n' || (c == '\r' && p[i + 1] == '\n');
        if (col + 1 < ncols) {
            if (eol) return (uint32_t)(col + 2) << 8 | BAD_MISSING;
            if (c != sep) return (uint32_t)(col + 1) << 8 | BAD_CELL;
            ++i;
        } else if (!eol) {
            return c == sep ? (uint32_t)(ncols + 1) << 8 | BAD_EXTRA : (uint32_t)(col + 1) << 8 | BAD_CELL;
        }
        cols[(int64_t)col * stride + row] = v;
    }
    return 0;
}

// One row per thread, adjacent lanes adjacent rows.  STAGED: the block first copies the text of its 256 rows into LDS with 128-bit loads (adjacent lanes
// adjacent 16 bytes) and the threads walk their rows there; a block whose rows span more than TSV_STAGE bytes reads global memory like the other form.
template <bool STAGED>
__global__ __launch_bounds__(TSV_BLOCK) void k_tsv_parse(const uint8_t *__restrict__ buf, uint32_t n, const uint32_t *__restrict__ starts, uint32_t nrows, int ncols,
                                                         uint8_t sep, double *__restrict__ cols, int64_t stride, int64_t row0, TsvResult *__restrict__ res,
                                                         uint2 *__restrict__ slow) {
    __shared__ uint32_t sh_not_int;
    __shared__ uint4 tile[STAGED ? TSV_STAGE / 16 + 1 : 1];
    if (threadIdx.x == 0) sh_not_int = 0;
    const uint32_t r0 = blockIdx.x * TSV_BLOCK, r = r0 + threadIdx.x;
    uint32_t lo = 0;
    bool staged = false;
    if (STAGED) {
        const uint32_t r1 = min(r0 + TSV_BLOCK, nrows);
        lo = starts[r0] & ~15u;
        const uint32_t hi = r1 < nrows ? starts[r1] : n;   // (the byte before the next block's first row is a '\n': every row of this one ends below hi)
        staged = hi - lo <= TSV_STAGE;
        if (staged)
            for (uint32_t k = threadIdx.x; k < (hi - lo + 15) / 16 + 1; k += TSV_BLOCK) tile[k] = *reinterpret_cast<const uint4 *>(buf + lo + 16 * k);
    }
    __syncthreads();
    uint32_t not_int = 0;
    if (r < nrows) {
        const uint32_t s = starts[r];
        const uint32_t nxt = r + 1 < nrows ? starts[r + 1] : n;
        uint32_t bad = 0;
        if (nxt - s > (uint32_t)TSV_LINE_MAX) {   // (rare: a long line, or a run of empty lines behind this one)
            uint32_t e = s;
            while (buf[e] != '\n') ++e;
            if (e - s > (uint32_t)TSV_LINE_MAX) bad = 1u << 8 | BAD_LONG;
        }
        if (!bad) {
            if (STAGED && staged)
                bad = parse_row(reinterpret_cast<const uint8_t *>(tile) + (s - lo), ncols, sep, cols, stride, row0 + r, r, s, &res->slow, slow, &not_int);
            else
                bad = parse_row(buf + s, ncols, sep, cols, stride, row0 + r, r, s, &res->slow, slow, &not_int);
        }
        if (bad) atomicMin(&res->bad, (unsigned long long)r << 16 | bad);
    }
    if (not_int) atomicOr(&sh_not_int, not_int);
    __syncthreads();
    if (threadIdx.x == 0 && sh_not_int) atomicOr(&res->not_int, sh_not_int);
}

__global__ __launch_bounds__(256) void k_tsv_init(TsvResult *res, uint32_t keep_not_int, const uint32_t *__restrict__ off, uint32_t nblocks) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        res->bad = ~0ull;
        res->slow = 0;
        if (!keep_not_int) res->not_int = 0;
        res->rows = off[nblocks];   // the exclusive sums end with the total
    }
}

__global__ __launch_bounds__(256) void k_tsv_patch(const uint32_t *__restrict__ cell, const double *__restrict__ val, uint32_t n, int ncols, double *__restrict__ cols,
                                                   int64_t stride, int64_t row0) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k < n) cols[(int64_t)(cell[k] % (uint32_t)ncols) * stride + row0 + cell[k] / (uint32_t)ncols] = val[k];
}

// ---- ldw_links_load ---------------------------------------------------------------------------------------------------------------------------

// keep[i] = the row stays (its min_len_col value is not below min_len); for those: idx1 / idx2 = SNP index of pos1 / pos2 (the first SNP at that position:
// srt = positions ascending, order = the SNP of every sorted position, null when POS itself ascends).  bad = min of row << 8 | file column << 4 | reason:
// the leftmost fault of the earliest bad row.
__global__ __launch_bounds__(256) void k_links_map(const double *__restrict__ p1, const double *__restrict__ p2, const double *__restrict__ len, double min_len, int64_t n,
                                                   const int32_t *__restrict__ srt, const int32_t *__restrict__ order, int32_t L, uint32_t col1, uint32_t col2, uint32_t *__restrict__ keep,
                                                   int32_t *__restrict__ idx1, int32_t *__restrict__ idx2, unsigned long long *__restrict__ bad) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const bool k = len == nullptr || !(len[i] < min_len);
        keep[i] = k;
        if (!k) continue;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const double v = e ? p2[i] : p1[i];
            uint32_t why = 0;
            int32_t at = 0;
            if (!(v == floor(v)) || isinf(v)) {
                why = POS_FRACTION;
            } else if (v < -2147483648.0 || v > 2147483647.0) {
                why = POS_RANGE;
            } else {
                const int32_t q = (int32_t)v;
                at = (int32_t)lower_bound_dev<int32_t>(srt, L, q);
                if (at >= L || srt[at] != q) why = POS_UNKNOWN;
                else if (order) at = order[at];
            }
            if (why) atomicMin(bad, (unsigned long long)i << 8 | (e ? col2 : col1) << 4 | why);
            (e ? idx2 : idx1)[i] = at;
        }
    }
}

__global__ __launch_bounds__(256) void k_links_compact(const uint32_t *__restrict__ keep, const uint32_t *__restrict__ off, const int32_t *__restrict__ idx1,
                                                       const int32_t *__restrict__ idx2, const double *__restrict__ mi, int64_t n, int32_t *__restrict__ a,
                                                       int32_t *__restrict__ b, double *__restrict__ out_mi) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        if (keep[i]) {
            const uint32_t j = off[i];
            a[j] = idx2[i];   // from side = pos2
            b[j] = idx1[i];   // to side = pos1 (R/computePairwiseMI.R:319-320)
            out_mi[j] = mi[i];
        }
}

// ---- the reader's state -----------------------------------------------------------------------------------------------------------------------

struct TsvState {
    // what a pass over a text file borrows (TsvPass)
    PinnedPair pin;                      // pinned chunk buffers: TSV_FRONT '\n', the data, TSV_TAIL '\n'
    DevBuf img, cnt, off, starts, scan_tmp;
    PinnedBuf pin_rows;                  // uint32: the line count of the chunk in flight
    Event pass_ev[3];                    // before / after a chunk's copy, after its line count
    // the reader's own
    PinnedBuf pin_res;                   // TsvResult [2]: pinned twin of res, one per chunk buffer
    DevBuf slow, res, patch;
    DevBuf cols;                         // double [ncols][stride], column-major: the parsed table
    int64_t rows = 0, stride = 0;
    int ncols = 0;
    int64_t grows = 0;                   // times the columns were moved to a larger buffer (since the context was made)
    Event ev[2][2];                      // per chunk buffer: before / after the parse kernel
    std::string path;                    // of the last read, for the line numbers of ldw_links_load's refusals
    int variant = 0;                     // 0: rows parsed from cached global loads, 1: from an LDS-staged tile
    double ms[8] = {};                   // last read: total, read (host), copy, line kernels, parse kernel, slow-cell patch, chunks, bytes
    DevBuf keep, koff, idx1, idx2, bad;   // ldw_links_load
};

TsvState *tsv_state(ldw_ctx *c) {
    if (!c->tsv) c->tsv = new TsvState();
    return static_cast<TsvState *>(c->tsv);
}

// room for `rows` rows: the columns move to a buffer of a larger stride (every column by one device-to-device copy)
int grow_columns(ldw_ctx *c, TsvState *t, int64_t rows) {
    if (rows <= t->stride && t->cols.p) return LDW_OK;
    int64_t stride = std::max<int64_t>(rows, t->stride + t->stride / 2);
    stride = (stride + 1023) / 1024 * 1024;
    if ((size_t)stride * 8 * (size_t)t->ncols <= t->cols.cap && t->rows == 0) {   // (an empty table has nothing to move: the buffer it has is re-cut)
        t->stride = (int64_t)(t->cols.cap / 8 / (size_t)t->ncols);
        return LDW_OK;
    }
    DevBuf nb;
    if (int rc = nb.reserve((size_t)stride * 8 * (size_t)t->ncols)) return rc;
    if (t->rows > 0) {
        LDW_HIP(hipMemcpy2DAsync(nb.p, (size_t)stride * 8, t->cols.p, (size_t)t->stride * 8, (size_t)t->rows * 8, (size_t)t->ncols, hipMemcpyDeviceToDevice, c->stream));
        LDW_HIP(hipStreamSynchronize(c->stream));
    }
    t->cols = std::move(nb);
    t->stride = stride;
    ++t->grows;
    return LDW_OK;
}

}  // namespace

namespace ldw {
void tsv_release(ldw_ctx *c) { release_state<TsvState>(c, c->tsv); }

// ---- TsvPass, the stream half (the host half: ldw_links_read_host.cpp) --------------------------------------------------------------------------

int TsvPass::attach(ldw_ctx *c) {
    ctx_ = c;
    TsvState *t = tsv_state(c);
    for (auto &e : t->pass_ev) LDW_HIP(e.ensure());
    if (int rc = t->pin_rows.reserve(4, "ldw_tsv_read")) return rc;
    const size_t buf_bytes = (size_t)buffer_bytes();
    if (int rc = t->pin.reserve(buf_bytes, "ldw_tsv_read")) return rc;   // (the pair is the reader's, whoever asks)
    if (int rc = t->img.reserve(buf_bytes)) return rc;
    const int64_t max_blocks = (cap_ + TSV_TILE - 1) / TSV_TILE + 1;
    if (int rc = t->cnt.reserve((size_t)(max_blocks + 1) * 4)) return rc;
    if (int rc = t->off.reserve((size_t)(max_blocks + 1) * 4)) return rc;
    size_t scan_bytes = 0;
    LDW_HIP(prim_scan_bytes<uint32_t>((size_t)max_blocks + 1, c->stream, &scan_bytes));
    if (int rc = t->scan_tmp.reserve(scan_bytes)) return rc;
    d_text_ = t->img.as<uint8_t>() + TSV_FRONT;
    use(t->pin.b[0], t->pin.b[1]);
    return LDW_OK;
}

int TsvPass::queue() {
    TsvState *t = tsv_state(ctx_);
    hipStream_t s = ctx_->stream;
    const int64_t cut = cut_, padded = (cut + 15) / 16 * 16;   // (the kernels load 16 bytes at a time)
    const uint32_t nblocks = (uint32_t)((cut + TSV_TILE - 1) / TSV_TILE);
    LDW_HIP(hipEventRecord(t->pass_ev[0], s));
    LDW_HIP(hipMemcpyAsync(t->img.p, buf_[buffer()], (size_t)(TSV_FRONT + padded + TSV_TAIL - 16), hipMemcpyHostToDevice, s));
    LDW_HIP(hipEventRecord(t->pass_ev[1], s));
    LDW_HIP(hipMemsetAsync(t->cnt.as<uint32_t>() + nblocks, 0, 4, s));
    LDW_LAUNCH(k_tsv_count, dim3(nblocks), dim3(TSV_BLOCK), 0, s, d_text_, (uint32_t)cut, t->cnt.as<uint32_t>());
    size_t sb = t->scan_tmp.cap;
    LDW_HIP(prim_exclusive_sum(t->scan_tmp.p, sb, t->cnt.as<uint32_t>(), t->off.as<uint32_t>(), (size_t)nblocks + 1, s));
    d_rows_ = t->off.as<uint32_t>() + nblocks;   // the exclusive sums end with the total
    LDW_HIP(hipMemcpyAsync(t->pin_rows, d_rows_, 4, hipMemcpyDeviceToHost, s));
    LDW_HIP(hipEventRecord(t->pass_ev[2], s));
    return LDW_OK;
}

int TsvPass::wait(uint32_t *rows) {
    TsvState *t = tsv_state(ctx_);
    LDW_HIP(hipEventSynchronize(t->pass_ev[2]));
    float f = 0;
    if (hipEventElapsedTime(&f, t->pass_ev[0], t->pass_ev[1]) == hipSuccess) copy_ms += f;
    if (hipEventElapsedTime(&f, t->pass_ev[1], t->pass_ev[2]) == hipSuccess) line_ms += f;
    *rows = *t->pin_rows.as<uint32_t>();
    return LDW_OK;
}

int TsvPass::starts(uint32_t rows, const uint32_t **d_starts) {
    TsvState *t = tsv_state(ctx_);
    const uint32_t nblocks = (uint32_t)((cut_ + TSV_TILE - 1) / TSV_TILE);
    if (int rc = t->starts.reserve((size_t)std::max<uint32_t>(rows, 1) * 4)) return rc;
    LDW_LAUNCH(k_tsv_starts, dim3(nblocks), dim3(TSV_BLOCK), 0, ctx_->stream, d_text_, (uint32_t)cut_, t->off.as<uint32_t>(), t->starts.as<uint32_t>());
    *d_starts = t->starts.as<uint32_t>();
    return LDW_OK;
}

void TsvPass::drain() { (void)hipStreamSynchronize(ctx_->stream); }

int64_t tsv_trim(ldw_ctx *c) {
    auto *t = static_cast<TsvState *>(c->tsv);
    if (!t) return 0;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    const int64_t n = t->pin.release() + (int64_t)t->img.cap;
    t->img.release();
    return n;
}
}  // namespace ldw

extern "C" {

int ldw_tsv_read(ldw_ctx *c, const char *path, int sep, int32_t ncols, int64_t chunk_bytes, int64_t *rows_out, int64_t *slow_cells_out, uint32_t *int_cols_mask_out) {
    if (rows_out) *rows_out = 0;
    if (slow_cells_out) *slow_cells_out = 0;
    if (int_cols_mask_out) *int_cols_mask_out = 0;
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(path != nullptr, LDW_ERR_ARG, "ldw_tsv_read: null path");
    LDW_REQUIRE(sep == '\t' || sep == ' ', LDW_ERR_ARG, "ldw_tsv_read: the separator must be a tab or a space (got %d)", sep);
    LDW_REQUIRE(ncols >= 1 && ncols <= TSV_MAX_COLS, LDW_ERR_ARG, "ldw_tsv_read: ncols = %d outside 1..%d", (int)ncols, TSV_MAX_COLS);
    TsvPass pass("ldw_tsv_read", path);
    if (int rc = pass.open(chunk_bytes)) return rc;
    TsvState *t = tsv_state(c);
    t->rows = 0;
    t->path = path;
    if (t->ncols != ncols) t->stride = 0;   // (the buffer is cut anew: grow_columns)
    t->ncols = ncols;
    memset(t->ms, 0, sizeof(t->ms));
    const auto t_begin = std::chrono::steady_clock::now();
    for (auto &row : t->ev)
        for (auto &e : row) LDW_HIP(e.ensure());
    if (int rc = t->pin_res.reserve(2 * sizeof(TsvResult), "ldw_tsv_read")) return rc;
    if (int rc = t->res.reserve(sizeof(TsvResult))) return rc;
    if (int rc = pass.attach(c)) return rc;

    int rc = LDW_OK;
    int64_t slow_total = 0, file_bytes = 0;
    uint32_t bad_reason = 0, bad_col = 0;
    int64_t bad_row = -1;
    struct Chunk {
        int64_t row0 = 0;
        bool queued = false;
    } ch[2];
    TsvResult *d_res = t->res.as<TsvResult>();

    // waits for a chunk's kernels; converts and patches its slow cells from the pinned text; notes its first refused row
    auto finish = [&](int b) -> int {
        Chunk &k = ch[b];
        if (!k.queued) return LDW_OK;
        k.queued = false;
        hipError_t e = hipEventSynchronize(t->ev[b][1]);
        if (e != hipSuccess) return hip_fail(e, "ldw_tsv_read: chunk", __FILE__, __LINE__);
        const TsvResult r = t->pin_res.as<TsvResult>()[b];
        float f = 0;
        if (hipEventElapsedTime(&f, t->ev[b][0], t->ev[b][1]) == hipSuccess) t->ms[4] += f;
        if (r.bad != ~0ull) {
            bad_row = k.row0 + (int64_t)(r.bad >> 16);
            bad_col = (uint32_t)(r.bad >> 8) & 0xff;
            bad_reason = (uint32_t)r.bad & 0xff;
            return LDW_ERR_ARG;
        }
        if (r.slow > 0) {
            const auto p0 = std::chrono::steady_clock::now();
            std::vector<uint2> list(r.slow);
            LDW_HIP(hipMemcpyAsync(list.data(), t->slow.p, (size_t)r.slow * 8, hipMemcpyDeviceToHost, c->stream));
            LDW_HIP(hipStreamSynchronize(c->stream));
            // [cells (uint32) | values (double)] in one buffer, one copy
            const size_t voff = ((size_t)r.slow * 4 + 7) / 8 * 8;
            std::vector<unsigned char> host(voff + (size_t)r.slow * 8);
            uint32_t *cell = reinterpret_cast<uint32_t *>(host.data());
            double *val = reinterpret_cast<double *>(host.data() + voff);
            const char *text = pass.text(b);
            for (uint32_t i = 0; i < r.slow; ++i) {
                cell[i] = list[i].x;
                val[i] = tsv_strtod(text + list[i].y);
            }
            if (int rc2 = t->patch.reserve(host.size())) return rc2;
            LDW_HIP(hipMemcpyAsync(t->patch.p, host.data(), host.size(), hipMemcpyHostToDevice, c->stream));
            LDW_LAUNCH(k_tsv_patch, dim3((r.slow + 255) / 256), dim3(256), 0, c->stream, t->patch.as<uint32_t>(),
                               reinterpret_cast<const double *>(t->patch.as<unsigned char>() + voff), r.slow, t->ncols, t->cols.as<double>(), t->stride, k.row0);
            LDW_HIP(hipStreamSynchronize(c->stream));   // (`host` goes out of scope)
            t->ms[5] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - p0).count();
            slow_total += r.slow;
        }
        return LDW_OK;
    };
    // a chunk's rows, counted, into the columns: k_tsv_starts and the parse kernel, not waited for
    auto parse = [&](int b, uint32_t nrows) -> int {
        int64_t want = t->rows + nrows;
        if (pass.nchunks == 1 && file_bytes > pass.cut())   // a plain file: sized once from its first chunk
            want = std::max<int64_t>(want, (int64_t)((double)nrows * ((double)file_bytes / (double)pass.cut()) * 1.02) + 1024);
        if (int rc2 = grow_columns(c, t, want)) return rc2;
        if (int rc2 = t->slow.reserve((size_t)nrows * (size_t)ncols * 8)) return rc2;
        LDW_HIP(hipEventRecord(t->ev[b][0], c->stream));
        const uint32_t *d_starts = nullptr;
        if (int rc2 = pass.starts(nrows, &d_starts)) return rc2;
        const dim3 grid((nrows + TSV_BLOCK - 1) / TSV_BLOCK);
        if (t->variant == 1)
            LDW_LAUNCH(k_tsv_parse<true>, grid, dim3(TSV_BLOCK), 0, c->stream, pass.d_text(), (uint32_t)pass.cut(), d_starts, nrows, (int)ncols, (uint8_t)sep,
                       t->cols.as<double>(), t->stride, t->rows, d_res, t->slow.as<uint2>());
        else
            LDW_LAUNCH(k_tsv_parse<false>, grid, dim3(TSV_BLOCK), 0, c->stream, pass.d_text(), (uint32_t)pass.cut(), d_starts, nrows, (int)ncols, (uint8_t)sep,
                       t->cols.as<double>(), t->stride, t->rows, d_res, t->slow.as<uint2>());
        LDW_HIP(hipMemcpyAsync(t->pin_res.as<TsvResult>() + b, d_res, sizeof(TsvResult), hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipEventRecord(t->ev[b][1], c->stream));
        ch[b].row0 = t->rows;
        ch[b].queued = true;
        t->rows += nrows;
        return LDW_OK;
    };

    if (pass.more() && !pass.gzip()) {
        FileStamp st;
        if (file_stamp(path, &st) == LDW_OK) file_bytes = st.size;
    }
    for (; rc == LDW_OK && pass.more(); pass.advance()) {
        const int b = pass.buffer();
        // the chunk before this one: the other buffer still holds the text of its slow cells, and takes this one's carried line next
        if ((rc = finish(1 - b))) break;
        pass.begin();
        if ((rc = pass.queue())) break;
        hipLaunchKernelGGL(k_tsv_init, dim3(1), dim3(256), 0, c->stream, d_res, (uint32_t)(pass.nchunks > 1), pass.d_rows(), 0u);
        if (hipError_t e = hipGetLastError()) {
            rc = hip_fail(e, "ldw_tsv_read: k_tsv_init", __FILE__, __LINE__);
            break;
        }
        // the next chunk is read while this one is copied and its lines are counted
        pass.prefetch();
        uint32_t nrows = 0;
        if ((rc = pass.wait(&nrows))) break;
        if (nrows > 0) rc = parse(b, nrows);
    }
    for (int b = 0; b < 2 && rc == LDW_OK; ++b) rc = finish(b);
    if (rc == LDW_OK) rc = pass.feeder_refusal();   // the feeder's own refusal comes after every row before it
    if (bad_row >= 0) rc = pass.refuse_row(bad_row, bad_col, bad_reason, ncols);
    uint32_t not_int = 0;
    if (rc == LDW_OK && pass.nchunks > 0) {
        hipError_t e = hipMemcpyAsync(&not_int, &d_res->not_int, 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = hip_fail(e, "ldw_tsv_read: result", __FILE__, __LINE__);
    }
    t->ms[2] = pass.copy_ms;
    t->ms[3] = pass.line_ms;
    if (rc != LDW_OK) {
        t->rows = 0;
        return rc;
    }
    t->ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    t->ms[1] = pass.read_ms();
    t->ms[6] = (double)pass.nchunks;
    t->ms[7] = (double)pass.consumed;
    if (rows_out) *rows_out = t->rows;
    if (slow_cells_out) *slow_cells_out = slow_total;
    if (int_cols_mask_out) *int_cols_mask_out = t->rows > 0 ? ~not_int & ((1u << ncols) - 1) : 0;
    return LDW_OK;
}

int ldw_tsv_columns(ldw_ctx *c, const double **device_ptr_out, int64_t *rows_out, int32_t *ncols_out, int64_t *stride_out) {
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(device_ptr_out && rows_out && ncols_out && stride_out, LDW_ERR_ARG, "ldw_tsv_columns: null argument");
    auto *t = static_cast<TsvState *>(c->tsv);
    LDW_REQUIRE(t && t->ncols > 0, LDW_ERR_STATE, "ldw_tsv_columns: no table has been read (ldw_tsv_read)");
    LDW_HIP(hipStreamSynchronize(c->stream));
    *device_ptr_out = t->rows > 0 ? t->cols.as<double>() : nullptr;
    *rows_out = t->rows;
    *ncols_out = t->ncols;
    *stride_out = t->stride;
    return LDW_OK;
}

int ldw_tsv_fetch(ldw_ctx *c, int32_t col, double *dst, int64_t capacity, int on_device) {
    if (int rc = check_gpu(c)) return rc;
    auto *t = static_cast<TsvState *>(c->tsv);
    LDW_REQUIRE(t && t->ncols > 0, LDW_ERR_STATE, "ldw_tsv_fetch: no table has been read (ldw_tsv_read)");
    LDW_REQUIRE(col >= 0 && col < t->ncols, LDW_ERR_ARG, "ldw_tsv_fetch: column %d outside 0..%d", (int)col, t->ncols - 1);
    LDW_REQUIRE(capacity >= t->rows, LDW_ERR_SIZE, "ldw_tsv_fetch: capacity %lld < %lld rows", (long long)capacity, (long long)t->rows);
    if (t->rows == 0) return LDW_OK;
    LDW_REQUIRE(dst != nullptr, LDW_ERR_ARG, "ldw_tsv_fetch: null output");
    LDW_HIP(hipMemcpyAsync(dst, t->cols.as<double>() + (int64_t)col * t->stride, (size_t)t->rows * 8, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    return LDW_OK;
}

int ldw_set_positions(ldw_ctx *c, const int32_t *POS, int64_t L, double g) {
    if (int rc = check_gpu(c)) return rc;
    if (int rc = join_prepare(c)) return rc;
    if (int rc = ldw_tsv_join(c)) return rc;   // (a pending asynchronous table reads the positions this call replaces)
    LDW_REQUIRE(POS != nullptr && L > 0 && L < ((int64_t)1 << 27), LDW_ERR_ARG, "ldw_set_positions: null positions or L = %lld outside 1..2^27", (long long)L);
    LDW_REQUIRE(g >= 0 && !std::isnan(g), LDW_ERR_ARG, "ldw_set_positions: genome length g must be positive, or 0 when it is not known");
    LDW_REQUIRE(c->links.blk_capacity == 0 && c->lr_stream == nullptr, LDW_ERR_STATE, "ldw_set_positions: a link pass or an lr_links stream is still open");
    LDW_HIP(hipStreamSynchronize(c->stream));
    if (int rc = c->meta.POS.reserve((size_t)L * 4)) return rc;
    LDW_HIP(hipMemcpyAsync(c->meta.POS.p, POS, (size_t)L * 4, hipMemcpyHostToDevice, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    // what an alignment would have brought is gone: states, weights, r, uqe and paint; the tables index the old SNPs
    c->L = L;
    c->N = c->Npad = c->KW = 0;
    c->positions_only();
    c->meta.h_r.clear();
    c->meta.h_paint.clear();
    c->meta.paint_min = c->meta.paint_max = 0;
    c->meta.set_positions(POS, L);
    c->meta.g = g;
    c->meta.mark_set(true);
    return LDW_OK;
}

int ldw_links_load(ldw_ctx *c, int which, int32_t pos1_col, int32_t pos2_col, int32_t mi_col, int32_t min_len_col, double min_len, int32_t flags, int64_t *n_out) {
    if (n_out) *n_out = 0;
    if (int rc = check_gpu(c)) return rc;
    if (int rc = join_prepare(c)) return rc;
    LDW_REQUIRE(which == 0 || which == 1, LDW_ERR_ARG, "ldw_links_load: which must be 0 (sr) or 1 (lr)");
    LDW_REQUIRE(flags == 0, LDW_ERR_ARG, "ldw_links_load: flags must be 0");
    auto *t = static_cast<TsvState *>(c->tsv);
    LDW_REQUIRE(t && t->ncols > 0, LDW_ERR_STATE, "ldw_links_load: no table has been read (ldw_tsv_read)");
    const int nc = t->ncols;
    LDW_REQUIRE(pos1_col >= 0 && pos1_col < nc && pos2_col >= 0 && pos2_col < nc && mi_col >= 0 && mi_col < nc && min_len_col >= -1 && min_len_col < nc, LDW_ERR_ARG,
                "ldw_links_load: a column index lies outside the %d columns read (min_len_col: -1 for none)", nc);
    LDW_REQUIRE(c->meta.have_meta && c->meta.POS.p && (int64_t)c->meta.h_POS.size() == c->L, LDW_ERR_STATE, "ldw_links_load: no positions (ldw_set_snp_meta or ldw_set_positions)");
    LDW_REQUIRE(c->links.blk_capacity == 0, LDW_ERR_STATE, "ldw_links_load: a link pass is still open (ldw_links_end)");
    const int64_t n = t->rows, L = c->L;
    LDW_REQUIRE(n < 2147483647LL, LDW_ERR_SIZE, "ldw_links_load: too many rows");
    if (c->gemm_stream) LDW_HIP(hipStreamSynchronize(c->gemm_stream));
    DevBuf &A = which == 0 ? c->links.sr_a : c->links.lr_a, &B = which == 0 ? c->links.sr_b : c->links.lr_b, &M = which == 0 ? c->links.sr_mi : c->links.lr_mi;
    int64_t kept = 0;
    if (n > 0) {
        // the positions in ascending order: POS itself, or the context's sorted copy with the SNP of every entry (the first SNP of a position first)
        const int32_t *d_srt = c->meta.POS.as<int32_t>(), *d_order = nullptr;
        if (!c->meta.pos_sorted) {
            if (int rc = pos_order(c)) return rc;
            d_srt = c->meta.pos_ord.srt.as<int32_t>();
            d_order = c->meta.pos_ord.order.as<int32_t>();
        }
        if (int rc = t->keep.reserve((size_t)(n + 1) * 4)) return rc;
        if (int rc = t->koff.reserve((size_t)(n + 1) * 4)) return rc;
        if (int rc = t->idx1.reserve((size_t)n * 4)) return rc;
        if (int rc = t->idx2.reserve((size_t)n * 4)) return rc;
        if (int rc = t->bad.reserve(8)) return rc;
        size_t sb = 0;
        LDW_HIP(prim_scan_bytes<uint32_t>((size_t)n + 1, c->stream, &sb));
        if (int rc = t->scan_tmp.reserve(sb)) return rc;
        sb = t->scan_tmp.cap;
        const double *cols = t->cols.as<double>();
        LDW_HIP(hipMemsetAsync(t->bad.p, 0xff, 8, c->stream));
        LDW_HIP(hipMemsetAsync(t->keep.as<uint32_t>() + n, 0, 4, c->stream));
        LDW_LAUNCH(k_links_map, grid_of(n), dim3(256), 0, c->stream, cols + (int64_t)pos1_col * t->stride, cols + (int64_t)pos2_col * t->stride,
                           min_len_col >= 0 ? cols + (int64_t)min_len_col * t->stride : nullptr, min_len, n, d_srt, d_order, (int32_t)L, (uint32_t)pos1_col, (uint32_t)pos2_col, t->keep.as<uint32_t>(),
                           t->idx1.as<int32_t>(), t->idx2.as<int32_t>(), t->bad.as<unsigned long long>());
        LDW_HIP(prim_exclusive_sum(t->scan_tmp.p, sb, t->keep.as<uint32_t>(), t->koff.as<uint32_t>(), (size_t)n + 1, c->stream));
        unsigned long long bad = 0;
        uint32_t total = 0;
        LDW_HIP(hipMemcpyAsync(&bad, t->bad.p, 8, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipMemcpyAsync(&total, t->koff.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipStreamSynchronize(c->stream));
        if (bad != ~0ull) {
            const int64_t row = (int64_t)(bad >> 8);
            const int bad_col = (int)(bad >> 4) & 15, why = (int)bad & 15;
            double v = 0;
            LDW_HIP(hipMemcpy(&v, cols + (int64_t)bad_col * t->stride + row, 8, hipMemcpyDeviceToHost));
            int64_t line = 0;
            (void)tsv_line_of_row(t->path.c_str(), row, &line);
            const int col = bad_col + 1;
            if (why == POS_FRACTION) set_error("ldw_links_load: %s: line %lld, column %d: the position %.17g is not an integer", t->path.c_str(), (long long)line, col, v);
            else if (why == POS_RANGE) set_error("ldw_links_load: %s: line %lld, column %d: the position %.17g does not fit in 32 bits", t->path.c_str(), (long long)line, col, v);
            else set_error("ldw_links_load: %s: line %lld, column %d: the position %.17g is no SNP's", t->path.c_str(), (long long)line, col, v);
            return LDW_ERR_ARG;
        }
        kept = total;
        if (int rc = A.reserve((size_t)std::max<int64_t>(kept, 1) * 4)) return rc;
        if (int rc = B.reserve((size_t)std::max<int64_t>(kept, 1) * 4)) return rc;
        if (int rc = M.reserve((size_t)std::max<int64_t>(kept, 1) * 8)) return rc;
        LDW_LAUNCH(k_links_compact, grid_of(n), dim3(256), 0, c->stream, t->keep.as<uint32_t>(), t->koff.as<uint32_t>(), t->idx1.as<int32_t>(), t->idx2.as<int32_t>(),
                           cols + (int64_t)mi_col * t->stride, n, A.as<int32_t>(), B.as<int32_t>(), M.as<double>());
        LDW_HIP(hipStreamSynchronize(c->stream));
    }
    (which == 0 ? c->links.n_sr : c->links.n_lr) = kept;
    c->links.replaced(c->kept);   // as ldw_links_import leaves the context
    if (n_out) *n_out = kept;
    return LDW_OK;
}

// ---- include/ldweaver_amd_debug.h ---------------------------------------------------------------------------------------------------------------

int ldw_tsv_stats(ldw_ctx *c, double *out10) {
    LDW_REQUIRE(c && out10, LDW_ERR_ARG, "ldw_tsv_stats: null argument");
    auto *t = static_cast<TsvState *>(c->tsv);
    for (int k = 0; k < 10; ++k) out10[k] = 0;
    if (!t) return LDW_OK;
    for (int k = 0; k < 8; ++k) out10[k] = t->ms[k];
    out10[8] = (double)t->grows;
    out10[9] = (double)(t->pin.cap * 2);
    return LDW_OK;
}

int ldw_tsv_set_variant(ldw_ctx *c, int variant) {
    LDW_REQUIRE(c != nullptr, LDW_ERR_ARG, "null context");
    LDW_REQUIRE(variant == 0 || variant == 1, LDW_ERR_ARG, "ldw_tsv_set_variant: 0 (rows from cached global loads) or 1 (from an LDS-staged tile)");
    tsv_state(c)->variant = variant;
    return LDW_OK;
}

}  // extern "C"
