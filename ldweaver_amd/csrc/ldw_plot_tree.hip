// The tree view on the device (include/ldweaver_amd.h 15): the tree as axis-aligned bars summed into a coverage image, the allele and
// metadata bands as area-weighted means of their tips' colours, both composed into one white canvas.
//
// Bars.  A bar is the half-open rectangle [x0, x1) x [y0, y1) in 1/16 pixel, relative to the panel's top-left corner.  It adds to every panel pixel
// its overlap area with that pixel in units of 1/256 pixel (0..256) by an integer atomic add into a uint32 image: integer sums do not depend on the
// order of the adds.  A pixel's ink is min(sum, 256) and every channel (255 (256 - ink) + fg ink + 128) >> 8.  At most 2^23 bars of at most 256 per
// pixel: the sum stays below 2^32.
//
// Work.  k_tree_count gives every bar the number of panel pixels it meets; behind rocPRIM's exclusive sum of those counts, pixel t of the whole list
// belongs to the bar b with off[b] <= t < off[b + 1] and is pixel t - off[b] of that bar's box, row by row.  k_tree_splat walks t = 0 .. off[n] in a
// grid-stride loop, so every thread takes the same number of pixels (within one) whichever bars they belong to — a caterpillar's connectors, O(tips x
// width) pixels between them, and a balanced tree's root connector are spread like everything else — and the 64 lanes of a wave add into consecutive
// pixels of a row wherever a bar is wider than a few pixels.  A wave looks its first pixel's bar up once (a binary search over off); a lane whose pixel
// lies in a later bar searches on from there.
//
// Bands.  levels[R][N]: in units where tip i spans [i W, (i + 1) W) and pixel column p spans [p N, (p + 1) N) (W = the band's width in pixels), the
// overlaps ov of a column with the tips sum to N and a channel is (sum of ov c[level] + N / 2) / N in int64.  k_tree_band_line computes that line once
// per band, k_tree_band_fill repeats it down the band's rows.
//
// Bounds: a splat pixel lies inside the bar's box clipped to the panel; a band pixel inside its rectangle, which the host checked against the canvas;
// tips i0 .. of a column satisfy i W < (p + 1) N <= N W, so i < N.
#include <algorithm>
#include <vector>

#include "ldw_plot_prim.h"

namespace ldw {
namespace {

constexpr int TREE_MAX_DIM = 8192, TREE_COORD = 1 << 20, TREE_MAX_BANDS = 1024, TREE_SPLAT_BLOCKS = 2048;
constexpr int64_t TREE_MAX_BARS = (int64_t)1 << 23, TREE_MAX_TIPS = (int64_t)1 << 24;

struct PixBox {
    int x, y, w, h;   // panel pixels; w = 0: none
};

// the panel pixels a bar meets: columns floor(x0 / 16) .. ceil(x1 / 16) - 1, rows likewise, clipped to the panel
__device__ __forceinline__ PixBox bar_box(const ldw_bar &b, int PW, int PH) {
    const int xa = max(b.x0 >> 4, 0), xb = min((b.x1 + 15) >> 4, PW);
    const int ya = max(b.y0 >> 4, 0), yb = min((b.y1 + 15) >> 4, PH);
    PixBox r;
    r.x = xa;
    r.y = ya;
    r.w = xb > xa && yb > ya ? xb - xa : 0;
    r.h = r.w ? yb - ya : 0;
    return r;
}

__global__ __launch_bounds__(256) void k_tree_count(const ldw_bar *__restrict__ bars, int64_t n, int PW, int PH, uint64_t *__restrict__ cnt) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i <= n; i += (int64_t)gridDim.x * 256) {
        uint64_t k = 0;
        if (i < n) {
            const PixBox r = bar_box(bars[i], PW, PH);
            k = (uint64_t)r.w * (uint64_t)r.h;
        }
        cnt[i] = k;   // cnt[n] = 0: the exclusive sum puts the total there
    }
}

// the last b in [lo, n) with off[b] <= t, given off[lo] <= t < off[n]
__device__ __forceinline__ int64_t bar_of(const uint64_t *__restrict__ off, int64_t lo, int64_t n, uint64_t t) {
    int64_t hi = n;   // off[hi] > t
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= t)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_tree_splat(const ldw_bar *__restrict__ bars, const uint64_t *__restrict__ off, int64_t n, int PW, int PH,
                                                    uint32_t *__restrict__ cov) {
    const uint64_t total = off[n];
    const int lane = threadIdx.x & 63;
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (uint64_t)gridDim.x * 256) {
        int64_t b = bar_of(off, 0, n, t - lane);   // the bar of the wave's first pixel: the same loads in every lane
        if (t >= off[b + 1]) b = bar_of(off, b + 1, n, t);
        const ldw_bar bar = bars[b];
        const PixBox r = bar_box(bar, PW, PH);
        const uint32_t local = (uint32_t)(t - off[b]);   // < w h <= 2^26
        const int px = r.x + (int)(local % (uint32_t)r.w), py = r.y + (int)(local / (uint32_t)r.w);
        const int ox = min(bar.x1, (px + 1) << 4) - max(bar.x0, px << 4);
        const int oy = min(bar.y1, (py + 1) << 4) - max(bar.y0, py << 4);
        atomicAdd(&cov[(size_t)py * PW + px], (uint32_t)(ox * oy));
    }
}

__global__ __launch_bounds__(256) void k_tree_colour(const uint32_t *__restrict__ cov, int PW, int PH, int X, int Y, int CW, uint32_t fg, uint8_t *__restrict__ canvas) {
    const int fr = (int)(fg >> 16 & 0xff), fgn = (int)(fg >> 8 & 0xff), fb = (int)(fg & 0xff);
    const int64_t np = (int64_t)PW * PH;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < np; i += (int64_t)gridDim.x * 256) {
        const int px = (int)(i % PW), py = (int)(i / PW);
        const int ink = (int)min(cov[i], 256u);
        uint8_t *o = canvas + ((size_t)(Y + py) * CW + (X + px)) * 3;
        o[0] = (uint8_t)((255 * (256 - ink) + fr * ink + 128) >> 8);
        o[1] = (uint8_t)((255 * (256 - ink) + fgn * ink + 128) >> 8);
        o[2] = (uint8_t)((255 * (256 - ink) + fb * ink + 128) >> 8);
    }
}

// line[r][p][3], p < rect[r].w: one thread per band and pixel column
__global__ __launch_bounds__(256) void k_tree_band_line(const uint8_t *__restrict__ levels, const uint32_t *__restrict__ pal, const int32_t *__restrict__ rect, int R, int64_t N,
                                                        int maxw, uint8_t *__restrict__ line) {
    const int64_t cells = (int64_t)R * maxw;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < cells; idx += (int64_t)gridDim.x * 256) {
        const int r = (int)(idx / maxw), p = (int)(idx % maxw);
        const int64_t W = rect[4 * r + 2];
        if (p >= W) continue;
        const int64_t lo = (int64_t)p * N, hi = lo + N;
        const uint8_t *lev = levels + (size_t)r * N;
        const uint32_t *c = pal + (size_t)r * 256;
        int64_t sr = 0, sg = 0, sb = 0;
        for (int64_t i = lo / W; i * W < hi; ++i) {
            const int64_t ov = min(hi, (i + 1) * W) - max(lo, i * W);
            const uint32_t rgb = c[lev[i]];
            sr += ov * (int64_t)(rgb >> 16 & 0xff);
            sg += ov * (int64_t)(rgb >> 8 & 0xff);
            sb += ov * (int64_t)(rgb & 0xff);
        }
        uint8_t *o = line + (size_t)idx * 3;
        o[0] = (uint8_t)((sr + N / 2) / N);
        o[1] = (uint8_t)((sg + N / 2) / N);
        o[2] = (uint8_t)((sb + N / 2) / N);
    }
}

// blockIdx.y = band: its line repeated down its rows
__global__ __launch_bounds__(256) void k_tree_band_fill(const uint8_t *__restrict__ line, const int32_t *__restrict__ rect, int maxw, int CW, uint8_t *__restrict__ canvas) {
    const int r = blockIdx.y;
    const int x = rect[4 * r], y = rect[4 * r + 1], w = rect[4 * r + 2], h = rect[4 * r + 3];
    const int64_t np = (int64_t)w * h;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < np; i += (int64_t)gridDim.x * 256) {
        const int p = (int)(i % w), j = (int)(i / w);
        const uint8_t *s = line + ((size_t)r * maxw + p) * 3;
        uint8_t *o = canvas + ((size_t)(y + j) * CW + (x + p)) * 3;
        o[0] = s[0];
        o[1] = s[1];
        o[2] = s[2];
    }
}

bool rects_meet(const int32_t *a, const int32_t *b) { return a[0] < b[0] + b[2] && b[0] < a[0] + a[2] && a[1] < b[1] + b[3] && b[1] < a[1] + a[3]; }

int check_tree(int W, int H, const int32_t *panel, const ldw_bar *bars, int64_t n_bars, uint32_t bar_rgb, const uint8_t *levels, int64_t n_tips, const uint32_t *palette,
               const int32_t *band_rect, int n_bands, const char *who) {
    LDW_REQUIRE(n_bars >= 0 && n_bars <= TREE_MAX_BARS, LDW_ERR_ARG, "%s: %lld bars (0..%lld)", who, (long long)n_bars, (long long)TREE_MAX_BARS);
    LDW_REQUIRE(W >= 1 && H >= 1 && W <= TREE_MAX_DIM && H <= TREE_MAX_DIM, LDW_ERR_ARG, "%s: a canvas of %d x %d pixels (1..%d each way)", who, W, H, TREE_MAX_DIM);
    LDW_REQUIRE(panel && (n_bars == 0 || bars) && bar_rgb <= 0xFFFFFFu, LDW_ERR_ARG, "%s: null panel or bar list, or a colour beyond 0xFFFFFF", who);
    LDW_REQUIRE(panel[0] >= 0 && panel[1] >= 0 && panel[2] >= 1 && panel[3] >= 1 && panel[0] <= W - panel[2] && panel[1] <= H - panel[3], LDW_ERR_ARG,
                "%s: the panel %d, %d, %d x %d is empty or leaves the canvas", who, panel[0], panel[1], panel[2], panel[3]);
    LDW_REQUIRE(n_bands >= 0 && n_bands <= TREE_MAX_BANDS, LDW_ERR_ARG, "%s: %d bands (0..%d)", who, n_bands, TREE_MAX_BANDS);
    LDW_REQUIRE(n_bands == 0 || (levels && palette && band_rect && n_tips >= 1 && n_tips <= TREE_MAX_TIPS), LDW_ERR_ARG, "%s: null band arrays, or %lld tips (1..%lld)", who,
                (long long)n_tips, (long long)TREE_MAX_TIPS);
    LDW_REQUIRE(n_bands == 0 || (int64_t)n_bands * n_tips <= ((int64_t)1 << 31), LDW_ERR_ARG, "%s: %d bands of %lld tips are more than 2^31 levels", who, n_bands,
                (long long)n_tips);
    for (int64_t i = 0; i < n_bars; ++i) {
        const ldw_bar &b = bars[i];
        const int lo = std::min(std::min(b.x0, b.y0), std::min(b.x1, b.y1)), hi = std::max(std::max(b.x0, b.y0), std::max(b.x1, b.y1));
        LDW_REQUIRE(lo >= -TREE_COORD && hi <= TREE_COORD, LDW_ERR_ARG, "%s: bar %lld has a coordinate outside +-%d", who, (long long)i, TREE_COORD);
        LDW_REQUIRE(b.x1 > b.x0 && b.y1 > b.y0, LDW_ERR_ARG, "%s: bar %lld is empty (x1 <= x0 or y1 <= y0)", who, (long long)i);
    }
    for (int r = 0; r < n_bands; ++r) {
        const int32_t *q = band_rect + 4 * r;
        LDW_REQUIRE(q[0] >= 0 && q[1] >= 0 && q[2] >= 1 && q[3] >= 1 && q[0] <= W - q[2] && q[1] <= H - q[3], LDW_ERR_ARG, "%s: band %d is empty or leaves the canvas", who, r);
        LDW_REQUIRE(!rects_meet(q, panel), LDW_ERR_ARG, "%s: band %d overlaps the panel", who, r);
        for (int s = 0; s < r; ++s) LDW_REQUIRE(!rects_meet(q, band_rect + 4 * s), LDW_ERR_ARG, "%s: bands %d and %d overlap", who, s, r);
    }
    return LDW_OK;
}

// the canvas rgb_out[H][W][3] (host): white, the bars inside the panel, the bands.  ms_out (may be NULL, 4 doubles): clear, bars, bands, colour
int tree_raster(ldw_ctx *c, int W, int H, const int32_t *panel, const ldw_bar *bars, int64_t n, uint32_t fg, const uint8_t *levels, int64_t N, const uint32_t *pal,
                const int32_t *rect, int R, uint8_t *rgb_out, double *ms_out, const char *who) {
    LDW_REQUIRE(rgb_out, LDW_ERR_ARG, "%s: null output", who);
    const int PX = panel[0], PY = panel[1], PW = panel[2], PH = panel[3];
    int maxw = 1;
    for (int r = 0; r < R; ++r) maxw = std::max(maxw, (int)rect[4 * r + 2]);
    size_t scan_bytes = 0;
    LDW_HIP(prim_scan_bytes<uint64_t>((size_t)n + 1, c->stream, &scan_bytes));
    Carve cv;
    auto d_bars = cv.take<ldw_bar>(n);
    auto d_cnt = cv.take<uint64_t>(n + 1);
    auto d_off = cv.take<uint64_t>(n + 1);
    auto d_tmp = cv.take<uint8_t>((int64_t)scan_bytes);
    auto d_cov = cv.take<uint32_t>((int64_t)PW * PH);
    auto d_lev = cv.take<uint8_t>((int64_t)R * N);
    auto d_pal = cv.take<uint32_t>((int64_t)R * 256);
    auto d_rect = cv.take<int32_t>((int64_t)R * 4);
    auto d_line = cv.take<uint8_t>((int64_t)R * maxw * 3);
    auto d_canvas = cv.take<uint8_t>((int64_t)W * H * 3);
    if (int rc = cv.reserve(c->plot_work)) return rc;
    PlotEvents<5> events;
    if (ms_out) LDW_HIP(events.create());
    const Event *ev = events.e;
    hipStream_t st = c->stream;
    if (n > 0) LDW_HIP(hipMemcpyAsync(d_bars, bars, (size_t)n * sizeof(ldw_bar), hipMemcpyHostToDevice, st));
    if (R > 0) {
        LDW_HIP(hipMemcpyAsync(d_lev, levels, (size_t)R * N, hipMemcpyHostToDevice, st));
        LDW_HIP(hipMemcpyAsync(d_pal, pal, (size_t)R * 256 * 4, hipMemcpyHostToDevice, st));
        LDW_HIP(hipMemcpyAsync(d_rect, rect, (size_t)R * 16, hipMemcpyHostToDevice, st));
    }
    if (ms_out) LDW_HIP(hipEventRecord(ev[0], st));
    LDW_HIP(hipMemsetAsync(d_cov, 0, (size_t)PW * PH * 4, st));
    LDW_HIP(hipMemsetAsync(d_canvas, 0xFF, (size_t)W * H * 3, st));
    if (ms_out) LDW_HIP(hipEventRecord(ev[1], st));
    if (n > 0) {
        LDW_LAUNCH(k_tree_count, grid_of(n + 1), dim3(256), 0, st, (const ldw_bar *)d_bars, n, PW, PH, (uint64_t *)d_cnt);
        LDW_HIP(prim_exclusive_sum(d_tmp, scan_bytes, (const uint64_t *)d_cnt, (uint64_t *)d_off, (size_t)n + 1, st));
        LDW_LAUNCH(k_tree_splat, dim3(TREE_SPLAT_BLOCKS), dim3(256), 0, st, (const ldw_bar *)d_bars, (const uint64_t *)d_off, n, PW, PH, (uint32_t *)d_cov);
    }
    if (ms_out) LDW_HIP(hipEventRecord(ev[2], st));
    if (R > 0) {
        LDW_LAUNCH(k_tree_band_line, grid_of((int64_t)R * maxw), dim3(256), 0, st, (const uint8_t *)d_lev, (const uint32_t *)d_pal, (const int32_t *)d_rect, R, N, maxw,
                   (uint8_t *)d_line);
        int maxpix = 1;
        for (int r = 0; r < R; ++r) maxpix = std::max(maxpix, (int)(rect[4 * r + 2] * rect[4 * r + 3]));
        LDW_LAUNCH(k_tree_band_fill, dim3(std::min((maxpix + 255) / 256, 1024), R), dim3(256), 0, st, (const uint8_t *)d_line, (const int32_t *)d_rect, maxw, W,
                   (uint8_t *)d_canvas);
    }
    if (ms_out) LDW_HIP(hipEventRecord(ev[3], st));
    LDW_LAUNCH(k_tree_colour, grid_of((int64_t)PW * PH), dim3(256), 0, st, (const uint32_t *)d_cov, PW, PH, PX, PY, W, fg, (uint8_t *)d_canvas);
    if (ms_out) LDW_HIP(hipEventRecord(ev[4], st));
    LDW_HIP(hipMemcpyAsync(rgb_out, d_canvas, (size_t)W * H * 3, hipMemcpyDeviceToHost, st));
    LDW_HIP(hipStreamSynchronize(st));
    if (ms_out) LDW_HIP(events.elapsed(ms_out));
    return LDW_OK;
}

}  // namespace
}  // namespace ldw

using namespace ldw;

extern "C" {

int ldw_plot_tree(ldw_ctx *c, int32_t W, int32_t H, const int32_t *panel, const ldw_bar *bars, int64_t n_bars, uint32_t bar_rgb, const uint8_t *levels, int64_t n_tips,
                  const uint32_t *palette, const int32_t *band_rect, int32_t n_bands, const char *const *band_label, const char *title,
                  const char *const *legend_title, const int32_t *legend_n, const char *const *legend_label, const uint32_t *legend_rgb, const int32_t *legend_xy,
                  int32_t text_scale, const char *png_path, uint8_t *rgb_out, int32_t *boxes_out) {
    LDW_REQUIRE(c != nullptr, LDW_ERR_ARG, "ldw_plot_tree: null context");
    LDW_REQUIRE(png_path || rgb_out, LDW_ERR_ARG, "ldw_plot_tree: neither a path nor a canvas to write to");
    if (int rc = check_tree(W, H, panel, bars, n_bars, bar_rgb, levels, n_tips, palette, band_rect, n_bands, "ldw_plot_tree")) return rc;
    LDW_REQUIRE(text_scale >= 1 && text_scale <= 64, LDW_ERR_ARG, "ldw_plot_tree: text scale %d outside 1..64", (int)text_scale);
    LDW_REQUIRE(legend_title && legend_n && legend_xy, LDW_ERR_ARG, "ldw_plot_tree: null legend arrays");
    int64_t entries = 0;
    for (int k = 0; k < 2; ++k) {
        LDW_REQUIRE(legend_n[k] >= 0 && legend_n[k] <= 256, LDW_ERR_ARG, "ldw_plot_tree: legend %d has %d entries (0..256)", k, (int)legend_n[k]);
        entries += legend_n[k];
    }
    LDW_REQUIRE(entries == 0 || (legend_label && legend_rgb), LDW_ERR_ARG, "ldw_plot_tree: null legend entries");
    for (int64_t k = 0; k < entries; ++k) LDW_REQUIRE(legend_label[k] != nullptr, LDW_ERR_ARG, "ldw_plot_tree: legend entry %lld has no label", (long long)k);
    if (int rc = check_gpu(c)) return rc;
    PlotCanvas canvas(rgb_out, W, H);
    if (int rc = tree_raster(c, W, H, panel, bars, n_bars, bar_rgb, levels, n_tips, palette, band_rect, n_bands, canvas.rgb, nullptr, "ldw_plot_tree")) return rc;
    plot_tree_overlay(canvas.rgb, W, H, band_rect, band_label, n_bands, title, legend_title, legend_n, legend_label, legend_rgb, legend_xy, text_scale, boxes_out);
    return canvas.finish(png_path);
}

int ldw_debug_plot_tree(ldw_ctx *c, int32_t W, int32_t H, const int32_t *panel, const ldw_bar *bars, int64_t n_bars, uint32_t bar_rgb, const uint8_t *levels,
                        int64_t n_tips, const uint32_t *palette, const int32_t *band_rect, int32_t n_bands, uint8_t *rgb_out, double *ms_out) {
    LDW_REQUIRE(c != nullptr, LDW_ERR_ARG, "ldw_debug_plot_tree: null context");
    if (int rc = check_tree(W, H, panel, bars, n_bars, bar_rgb, levels, n_tips, palette, band_rect, n_bands, "ldw_debug_plot_tree")) return rc;
    if (int rc = check_gpu(c)) return rc;
    return tree_raster(c, W, H, panel, bars, n_bars, bar_rgb, levels, n_tips, palette, band_rect, n_bands, rgb_out, ms_out, "ldw_debug_plot_tree");
}

}  // extern "C"
