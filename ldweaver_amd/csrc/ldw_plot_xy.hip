// The "xy" figures on the device (include/ldweaver_amd.h 12): c<i>_fit.png — black points under a red polyline — and
// CDS_clustering.png — points coloured by class, drawn in row order.
//
// Points.  ggplot draws geom_point in data order, so a pixel shows the class of the LARGEST row whose disc covers it.  The scatter's statistics
// and centre passes (ldw_plot.hip) run over the columns with the class in the panel slot: the centre pass takes the maximum of the key
// (row + 1) << 8 | cls per CENTRE pixel, k_xy_paint the maximum of the key image over the disc round every output pixel (ldw_plot_prim.h).  The
// colour is class_rgb[key & 0xFF]: no column is read by row.  Both maxima are order independent.
//
// Line.  k_xy_segments turns the vertices into pixel segments, one thread per vertex pair: entry i is the segment between the centre pixels
// of vertices i and i + 1 where both are finite, the single pixel of vertex i where it is finite and neither neighbour is, and nothing
// otherwise.  The line is opaque and of one colour, so a pixel needs to know only WHETHER a segment covers it: k_xy_paint's block walks the
// entries 256 at a time, keeps in LDS those whose box (inflated by ceil(w / 2)) meets its 32 x 32 tile, and every pixel tests the kept ones by
// the capsule rule 4 D2 <= w^2 in 64-bit integers (plot_capsule_covers).  A covered pixel takes line_rgb over whatever the points left.
//
// Bounds: a kept row's and a finite vertex's pixel lie in [0, W) x [0, H) by the clamps of plot_pixel (both lie inside the axis range, which is
// taken over both); the paint pass reads the key image only at in-panel coordinates (0 outside) and writes one RGB triple per in-panel pixel;
// the LDS list holds at most 256 entries per round, one per thread.  W, H <= 8192 and w <= 1024 keep every product of the coverage test below 2^62.
#include <algorithm>
#include <cmath>
#include <vector>

#include "ldw_plot_prim.h"

#pragma clang fp contract(off)

namespace ldw {
namespace {

constexpr int XY_MAX_DIM = 8192, XY_MAX_LINE_W = 1024;
constexpr int64_t XY_MAX_VERTS = 1 << 17;

struct XYSeg {
    int32_t x0, y0, x1, y1;   // x0 < 0: no entry
};

struct XYPaint {
    PlotDisc disc;
    PlotTicks ticks;
    uint32_t class_rgb[LDW_PLOT_MAX_CLASSES], line_rgb;
    int line_w;
};

// ---- vertices to pixel segments: thread i looks at vertices i - 1, i, i + 1 ------------------------------------------------------------------------------
__device__ __forceinline__ bool xy_finite(const double *vx, const double *vy, int64_t i, int64_t n) {
    return i >= 0 && i < n && isfinite(vx[i]) && isfinite(vy[i]);
}

__global__ void __launch_bounds__(256) k_xy_segments(const double *__restrict__ vx, const double *__restrict__ vy, int64_t n, const PlotGeom G, XYSeg *__restrict__ seg) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    XYSeg s{-1, -1, -1, -1};
    if (xy_finite(vx, vy, i, n)) {
        const int ax = plot_pixel(vx[i], G.x0, G.x1, G.W), ay = G.H - 1 - plot_pixel(vy[i], G.y0, G.y1, G.H);
        if (xy_finite(vx, vy, i + 1, n)) {
            s = XYSeg{ax, ay, plot_pixel(vx[i + 1], G.x0, G.x1, G.W), G.H - 1 - plot_pixel(vy[i + 1], G.y0, G.y1, G.H)};
        } else if (!xy_finite(vx, vy, i - 1, n)) {
            s = XYSeg{ax, ay, ax, ay};
        }
    }
    seg[i] = s;
}

// ---- paint: one block per 32 x 32 tile, one thread per pixel (four rows each): disc maximum -> class colour, then the line over it -------------------------
__global__ void __launch_bounds__(256) k_xy_paint(const PlotGeom G, const XYPaint P, const unsigned long long *__restrict__ img, const XYSeg *__restrict__ seg,
                                                  int64_t n_seg, uint8_t *__restrict__ rast) {
    extern __shared__ unsigned long long tile[];
    __shared__ XYSeg hit[256];
    __shared__ int n_hit;
    const int bx = blockIdx.x * PLOT_T, by = blockIdx.y * PLOT_T;
    plot_tile_load(tile, img, G.W, G.H, bx, by, P.disc.h);
    const int lx = threadIdx.x % PLOT_T, ly0 = threadIdx.x / PLOT_T;
    bool line[4] = {false, false, false, false};
    const int r = (P.line_w + 1) / 2;
    const int64_t w2 = (int64_t)P.line_w * P.line_w;
    for (int64_t base = 0; base < n_seg; base += 256) {
        __syncthreads();
        if (threadIdx.x == 0) n_hit = 0;
        __syncthreads();
        if (base + threadIdx.x < n_seg) {
            const XYSeg c = seg[base + threadIdx.x];
            if (c.x0 >= 0 && max(c.x0, c.x1) + r >= bx && min(c.x0, c.x1) - r < bx + PLOT_T && max(c.y0, c.y1) + r >= by && min(c.y0, c.y1) - r < by + PLOT_T)
                hit[atomicAdd(&n_hit, 1)] = c;   // (any order: coverage is an OR)
        }
        __syncthreads();
        const int m = n_hit;
        for (int j = 0; j < m; ++j) {
            const XYSeg c = hit[j];
#pragma unroll
            for (int q = 0; q < 4; ++q) line[q] = line[q] || plot_capsule_covers(c.x0, c.y0, c.x1, c.y1, w2, bx + lx, by + ly0 + 8 * q);
        }
    }
    __syncthreads();   // (the tile, when there are no segments)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int ly = ly0 + 8 * q, gx = bx + lx, gy = by + ly;
        if (gx >= G.W || gy >= G.H) continue;
        uint32_t rgb;
        if (line[q]) {
            rgb = P.line_rgb;
        } else {
            const unsigned long long m = plot_disc_max(tile, P.disc, lx, ly);
            rgb = m == 0 ? P.ticks.grid_or_background(gx, gy) : P.class_rgb[(int)(m & 0xFF)];   // (cls < n_classes <= LDW_PLOT_MAX_CLASSES by the centre pass)
        }
        plot_store_rgb(rast + ((size_t)gy * G.W + gx) * 3, rgb);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------------------

struct XYArgs {
    ColSrc cols;        // x, y and, in the panel slot, the class (NULL: class 0), as given
    PlotFeed<3> feed;   // the same three as host columns
    int64_t n;
    int on_device;
    const double *line_x, *line_y;   // host
    int64_t n_line;
    int D, n_classes, line_w;
    const ldw_plot_xy_opts *o;
};

int check_args(const double *x, const double *y, const uint8_t *cls, int64_t n, int on_device, const double *line_x, const double *line_y, int64_t n_line,
               const ldw_plot_xy_opts *o, XYArgs &a, const char *who) {
    LDW_REQUIRE(o, LDW_ERR_ARG, "%s: null options", who);
    LDW_REQUIRE(o->kind == LDW_PLOT_FIT || o->kind == LDW_PLOT_CDS, LDW_ERR_ARG, "%s: figure kind %d is no xy figure", who, o->kind);
    LDW_REQUIRE(n >= 0, LDW_ERR_ARG, "%s: n = %lld < 0", who, (long long)n);
    LDW_REQUIRE(n == 0 || (x && y), LDW_ERR_ARG, "%s: null x or y column", who);
    a.D = o->D == 0 ? 11 : o->D;
    LDW_REQUIRE(a.D >= 1 && a.D <= LDW_PLOT_MAX_D && (a.D & 1), LDW_ERR_ARG, "%s: the disc diameter D = %d must be odd and in 1..%d", who, a.D, LDW_PLOT_MAX_D);
    LDW_REQUIRE(o->n_classes >= 1 && o->n_classes <= LDW_PLOT_MAX_CLASSES, LDW_ERR_ARG, "%s: %d classes outside 1..%d", who, o->n_classes, LDW_PLOT_MAX_CLASSES);
    a.line_w = o->line_w == 0 ? 5 : o->line_w;
    LDW_REQUIRE(a.line_w >= 1 && a.line_w <= XY_MAX_LINE_W, LDW_ERR_ARG, "%s: the line width %d lies outside 1..%d", who, a.line_w, XY_MAX_LINE_W);
    LDW_REQUIRE(o->line_rgb <= 0xFFFFFFu, LDW_ERR_ARG, "%s: the line's colour lies beyond 0xFFFFFF", who);
    for (int k = 0; k < o->n_classes; ++k)
        LDW_REQUIRE(o->class_rgb[k] <= 0xFFFFFFu, LDW_ERR_ARG, "%s: the colour of class %d lies beyond 0xFFFFFF", who, k);
    LDW_REQUIRE(n_line >= 0 && n_line <= XY_MAX_VERTS && (n_line == 0 || (line_x && line_y)), LDW_ERR_ARG, "%s: %lld line vertices (0..%lld), or null vertex arrays", who,
                (long long)n_line, (long long)XY_MAX_VERTS);
    a.cols = ColSrc{x, y, nullptr, nullptr, cls};
    a.feed = PlotFeed<3>{{x, y, cls}, {8, 8, 1}};
    a.n = n;
    a.on_device = on_device;
    a.line_x = line_x;
    a.line_y = line_y;
    a.n_line = n_line;
    a.n_classes = o->n_classes;
    a.o = o;
    return LDW_OK;
}

// f(columns on the device, first row, rows): for every chunk of host columns, or once for device columns where they lie
template <class F> int each_rows(ldw_ctx *c, const XYArgs &a, F f) {
    if (a.n == 0) return LDW_OK;
    if (a.on_device) return f(a.cols, (int64_t)0, a.n);
    return a.feed.each_chunk(c, a.n, [&](const void *const *d, int64_t i0, int64_t m) {
        return f(ColSrc{(const double *)d[0], (const double *)d[1], nullptr, nullptr, (const uint8_t *)d[2]}, i0, m);
    });
}

struct XYStats {
    double xr[2] = {0, 1}, yr[2] = {0, 1};
    int64_t kept = 0, dropped = 0;
};

// the arrays of one render inside ctx->plot_work
struct XYWork {
    unsigned long long *keys;
    uint8_t *rast;
    double *part, *vx, *vy;
    XYSeg *seg;
    size_t bytes;
};

int reserve_work(ldw_ctx *c, const XYArgs &a, int W, int H, XYWork &w) {
    const size_t pixels = (size_t)W * H;
    Carve cv;
    auto keys = cv.take<unsigned long long>((int64_t)pixels);
    auto rast = cv.take<uint8_t>((int64_t)pixels * 3);
    auto part = cv.take<double>((int64_t)PLOT_MAX_BLOCKS * PLOT_NPART);
    auto vx = cv.take<double>(a.n_line);
    auto vy = cv.take<double>(a.n_line);
    auto seg = cv.take<XYSeg>(a.n_line);
    if (int rc = cv.reserve(c->plot_work)) return rc;
    w = XYWork{keys, rast, part, vx, vy, seg, cv.bytes};
    if (!a.on_device && a.n > 0)
        if (int rc = c->plot_cols.reserve(a.feed.chunk_bytes(a.n))) return rc;
    return LDW_OK;
}

// ranges of the kept rows and the finite line vertices; refuses a class out of range
int xy_stats(ldw_ctx *c, const XYArgs &a, const XYWork &w, XYStats &st, const char *who) {
    double v[PLOT_NPART] = {INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY, 0, 0, 0, 0};   // (plot_stats_accum)
    if (int rc = each_rows(c, a, [&](const ColSrc &s, int64_t, int64_t m) { return plot_stats_accum(c, s, m, a.n_classes, w.part, v); })) return rc;
    LDW_REQUIRE(v[8] == 0, LDW_ERR_ARG, "%s: a class lies outside 0..%d", who, a.n_classes - 1);
    st.kept = (int64_t)v[6];
    st.dropped = (int64_t)v[7];
    for (int64_t i = 0; i < a.n_line; ++i) {
        const double x = a.line_x[i], y = a.line_y[i];
        if (!(std::isfinite(x) && std::isfinite(y))) continue;
        v[0] = std::min(v[0], x);
        v[1] = std::max(v[1], x);
        v[2] = std::min(v[2], y);
        v[3] = std::max(v[3], y);
    }
    if (v[0] <= v[1]) {
        st.xr[0] = v[0] == 0 ? 0.0 : v[0];
        st.xr[1] = v[1] == 0 ? 0.0 : v[1];
        st.yr[0] = v[2] == 0 ? 0.0 : v[2];
        st.yr[1] = v[3] == 0 ? 0.0 : v[3];
    }
    return LDW_OK;
}

// key image -> raster of one panel of W x H pixels, left on the device in w.rast; ev (may be NULL): 4 events round the clear, the centre pass, the paint pass
int xy_raster(ldw_ctx *c, const XYArgs &a, const XYWork &w, int W, int H, const double xlim[2], const double ylim[2], int nxt, const int32_t *xt, int nyt,
              const int32_t *yt, const Event *ev) {
    const PlotGeom G{xlim[0], xlim[1], ylim[0], ylim[1], W, H, a.n_classes};
    XYPaint P{};
    P.disc = PlotDisc::make(a.D);
    P.ticks = PlotTicks::make(nxt, xt, nyt, yt);
    for (int k = 0; k < a.n_classes; ++k) P.class_rgb[k] = a.o->class_rgb[k];
    P.line_rgb = a.o->line_rgb;
    P.line_w = a.line_w;
    if (ev) LDW_HIP(hipEventRecord(ev[0], c->stream));
    LDW_HIP(hipMemsetAsync(w.keys, 0, (size_t)W * H * 8, c->stream));
    if (ev) LDW_HIP(hipEventRecord(ev[1], c->stream));
    if (int rc = each_rows(c, a, [&](const ColSrc &s, int64_t i0, int64_t m) { return plot_centre_classes(c, s, m, i0, G, w.keys); })) return rc;
    if (a.n_line > 0) {
        LDW_HIP(hipMemcpyAsync(w.vx, a.line_x, (size_t)a.n_line * 8, hipMemcpyHostToDevice, c->stream));
        LDW_HIP(hipMemcpyAsync(w.vy, a.line_y, (size_t)a.n_line * 8, hipMemcpyHostToDevice, c->stream));
        LDW_LAUNCH(k_xy_segments, dim3((unsigned)((a.n_line + 255) / 256)), dim3(256), 0, c->stream, (const double *)w.vx, (const double *)w.vy, a.n_line, G, w.seg);
    }
    if (ev) LDW_HIP(hipEventRecord(ev[2], c->stream));
    LDW_LAUNCH(k_xy_paint, dim3((W + PLOT_T - 1) / PLOT_T, (H + PLOT_T - 1) / PLOT_T), dim3(256), plot_tile_lds(P.disc), c->stream, G, P, (const unsigned long long *)w.keys,
               (const XYSeg *)w.seg, a.n_line, w.rast);
    if (ev) LDW_HIP(hipEventRecord(ev[3], c->stream));
    return LDW_OK;
}

}  // namespace
}  // namespace ldw

using namespace ldw;

extern "C" {

int ldw_plot_xy(ldw_ctx *c, const double *x, const double *y, const uint8_t *cls, int64_t n, int on_device, const double *line_x, const double *line_y,
                int64_t n_line, const ldw_plot_xy_opts *opts, const char *title, const char *xlab, const char *ylab, const char *png_path, uint8_t *rgb_out,
                int64_t *dropped_out) {
    LDW_REQUIRE(c != nullptr, LDW_ERR_ARG, "ldw_plot_xy: null context");
    XYArgs a;
    if (int rc = check_args(x, y, cls, n, on_device, line_x, line_y, n_line, opts, a, "ldw_plot_xy")) return rc;
    LDW_REQUIRE(png_path || rgb_out, LDW_ERR_ARG, "ldw_plot_xy: neither a path nor a canvas to write to");
    if (int rc = check_gpu(c)) return rc;
    ldw_plot_layout lay;
    if (int rc = ldw_plot_xy_layout_get(opts->kind, 1, 0, 1, 0, 1, &lay)) return rc;   // (panel size: independent of the ranges)
    const int W = lay.panel_w, H = lay.panel_h;
    XYWork w;
    if (int rc = reserve_work(c, a, W, H, w)) return rc;
    XYStats st;
    if (int rc = xy_stats(c, a, w, st, "ldw_plot_xy")) return rc;
    if (int rc = ldw_plot_xy_layout_get(opts->kind, 1, st.xr[0], st.xr[1], st.yr[0], st.yr[1], &lay)) return rc;
    if (int rc = xy_raster(c, a, w, W, H, lay.xlim, lay.ylim, lay.n_xticks, lay.xtick_px, lay.n_yticks, lay.ytick_px, nullptr)) return rc;
    std::vector<uint8_t> raster((size_t)W * H * 3);
    LDW_HIP(hipMemcpyAsync(raster.data(), w.rast, raster.size(), hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    if (dropped_out) *dropped_out = st.dropped;
    PlotCanvas canvas(rgb_out, lay.width, lay.height);
    plot_xy_frame(canvas.rgb, lay, opts->kind, raster.data(), title, xlab, ylab, opts->class_rgb, opts->n_classes);
    return canvas.finish(png_path);
}

int ldw_debug_plot_xy_panel(ldw_ctx *c, const double *x, const double *y, const uint8_t *cls, int64_t n, int on_device, const double *line_x,
                            const double *line_y, int64_t n_line, const ldw_plot_xy_opts *opts, int32_t W, int32_t H, uint8_t *rgb_out, double *stats_out,
                            double *ms_out) {
    const char *who = "ldw_debug_plot_xy_panel";
    LDW_REQUIRE(c != nullptr, LDW_ERR_ARG, "%s: null context", who);
    XYArgs a;
    if (int rc = check_args(x, y, cls, n, on_device, line_x, line_y, n_line, opts, a, who)) return rc;
    LDW_REQUIRE(W >= 1 && H >= 1 && W <= XY_MAX_DIM && H <= XY_MAX_DIM, LDW_ERR_ARG, "%s: a panel of %d x %d pixels (1..%d each way)", who, W, H, XY_MAX_DIM);
    LDW_REQUIRE(rgb_out, LDW_ERR_ARG, "%s: null output", who);
    if (int rc = check_gpu(c)) return rc;
    XYWork w;
    if (int rc = reserve_work(c, a, W, H, w)) return rc;
    PlotEvents<2> ev_stats;   // round the statistics pass
    PlotEvents<4> ev;         // round the clear, the centre pass, the paint pass
    if (ms_out) {
        LDW_HIP(ev_stats.create());
        LDW_HIP(ev.create());
    }
    XYStats st;
    if (ms_out) LDW_HIP(hipEventRecord(ev_stats.e[0], c->stream));
    if (int rc = xy_stats(c, a, w, st, who)) return rc;
    if (ms_out) LDW_HIP(hipEventRecord(ev_stats.e[1], c->stream));
    double xlim[2], ylim[2], tick[LDW_PLOT_MAX_TICKS];
    int32_t xt[LDW_PLOT_MAX_TICKS], yt[LDW_PLOT_MAX_TICKS], nxt = 0, nyt = 0;
    LDW_REQUIRE(plot_axis(st.xr[0], st.xr[1], W, 0, xlim, tick, xt, &nxt) == LDW_OK && plot_axis(st.yr[0], st.yr[1], H, 1, ylim, tick, yt, &nyt) == LDW_OK, LDW_ERR_ARG,
                "%s: the data ranges are not finite intervals", who);
    if (int rc = xy_raster(c, a, w, W, H, xlim, ylim, nxt, xt, nyt, yt, ms_out ? ev.e : nullptr)) return rc;
    LDW_HIP(hipMemcpyAsync(rgb_out, w.rast, (size_t)W * H * 3, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    if (ms_out) {
        LDW_HIP(ev_stats.elapsed(ms_out));
        LDW_HIP(ev.elapsed(ms_out + 1));
    }
    if (stats_out) {
        const double v[6] = {st.xr[0], st.xr[1], st.yr[0], st.yr[1], (double)st.kept, (double)st.dropped};
        memcpy(stats_out, v, sizeof(v));
    }
    return LDW_OK;
}

}  // extern "C"
