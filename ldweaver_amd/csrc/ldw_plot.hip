// The plots on the device (include/ldweaver_amd.h 12): a scatter rasteriser that draws no point twice and sorts nothing, and
// the LD map's heat map.
//
// ggplot draws opaque points in row order, so the colour of a pixel is the colour of the LAST point whose disc covers it: the maximum of the
// draw-order key over those points.  k_plot_centre takes that maximum per CENTRE pixel (one 64-bit atomicMax per row into the key image),
// k_plot_disc takes the maximum of the key image over the disc of offsets round every output pixel — the disc is symmetric, so that is the
// maximum over the points whose disc covers the pixel — and turns the winning key into a colour.  Both maxima are order independent: the
// picture is a function of the set of rows.
//
// Bounds: a kept row's pixel lies in [0, W) x [0, H) by the clamps of plot_pixel, its panel in [0, n_panels) by the test in the kernel (the
// statistics pass has already refused the call if any row's panel is out of range); the disc pass reads the key image only at in-panel
// coordinates and writes one RGB triple per in-panel pixel.
#include <algorithm>
#include <string>
#include <vector>

#include "ldw_plot_prim.h"

#pragma clang fp contract(off)

namespace ldw {
int ldmap_device(ldw_ctx *c, int32_t reducer, int32_t from, int32_t to, int64_t *n_pos_out, int32_t *reducer_out, int32_t *B_out, bool want,
                 int64_t capacity, const double **d_htm);   // ldw_post.hip

namespace {

constexpr uint64_t KEY_LAYER = 1ull << 63;
enum { KEY_SRP = 0, KEY_FIRST_ROW = 1, KEY_CLASS = 2 };   // the draw orders of the centre pass (see there)

// the context's kept links (ldw_sr_pvalues / ldw_lr_tukey): row of the link table, its SNPs' positions, srp_max, clust_c, ARACNE flags
struct CtxSrc {
    const int64_t *row;
    const int32_t *a, *b, *POS;
    const double *mi, *srp;
    const uint32_t *meta;
    const uint8_t *flags;
    double g;
    uint8_t lut[256];   // clust_c -> panel
    int facets;
    __device__ __forceinline__ bool has_srp() const { return srp != nullptr; }
    __device__ __forceinline__ double srp_at(int64_t i) const { return srp[i]; }
    __device__ __forceinline__ void get(int64_t i, PlotRow &r) const {
        const int64_t t = row[i];
        r.x = circ_len((double)POS[b[t]], (double)POS[a[t]], g);   // pos1 = to side, pos2 = from side (R/computePairwiseMI.R:319-330)
        r.y = mi[t];
        r.srp = srp ? srp[i] : 0.0;
        r.layer = flags ? (flags[i] != 0) : 1;
        r.panel = facets ? lut[meta[i] & 0xFF] : 0;
    }
};

__device__ __forceinline__ bool plot_keep(const PlotRow &r, bool has_srp) {
    return isfinite(r.x) && isfinite(r.y) && (!has_srp || (isfinite(r.srp) && r.srp >= 0.0));
}

// ---- statistics: ranges of the kept rows, range of srp over the kept layer-1 rows, counts; [block][PLOT_NPART] partials ----------------------
template <class Src>
__global__ void __launch_bounds__(256) k_plot_stats(const Src s, int64_t n, int n_panels, double *__restrict__ part) {
    double v[PLOT_NPART] = {INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY, 0, 0, 0, 0};   // x, y, srp (min, max), kept, dropped, bad panel
    const bool hs = s.has_srp();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        PlotRow r;
        s.get(i, r);
        if (r.panel < 0 || r.panel >= n_panels) v[8] = 1;
        if (!plot_keep(r, hs)) {
            v[7] += 1;
            continue;
        }
        v[6] += 1;
        v[0] = fmin(v[0], r.x);
        v[1] = fmax(v[1], r.x);
        v[2] = fmin(v[2], r.y);
        v[3] = fmax(v[3], r.y);
        if (hs && r.layer) {
            v[4] = fmin(v[4], r.srp);
            v[5] = fmax(v[5], r.srp);
        }
    }
    plot_partials_reduce<3, 4>(v, part);
}

__global__ void __launch_bounds__(256) k_plot_present(const uint32_t *__restrict__ meta, int64_t n, uint32_t *__restrict__ present) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) present[meta[i] & 0xFF] = 1u;
}

// ---- centre pass: one atomicMax per kept row -------------------------------------------------------------------------------------------------
// key, srp order:  ((layer << 63) | bits(srp)) + 1   (srp >= 0: its bit pattern orders like its value; -0.0 counts as 0)
// key, row order:  (layer << 63) | (n - row)         (the first row is on top)
// key, classes:    (row + 1) << 8 | panel            (the xy figures: the LAST row is on top, the panel slot holds the class, one panel)
template <class Src, int KEY, int PRECHECK>
__global__ void __launch_bounds__(256) k_plot_centre(const Src s, int64_t n, int64_t row0, int64_t n_total, const PlotGeom G,
                                                     unsigned long long *__restrict__ img) {   // rows row0 .. row0 + n - 1 of a table of n_total
    const bool hs = s.has_srp();
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        PlotRow r;
        s.get(i, r);
        if (!plot_keep(r, hs) || r.panel < 0 || r.panel >= G.n_panels) continue;
        const int px = plot_pixel(r.x, G.x0, G.x1, G.W), py = G.H - 1 - plot_pixel(r.y, G.y0, G.y1, G.H);
        const size_t at = ((size_t)(KEY == KEY_CLASS ? 0 : r.panel) * G.H + py) * G.W + px;
        unsigned long long key = r.layer ? KEY_LAYER : 0ull;
        if (KEY == KEY_CLASS)
            key = ((unsigned long long)(row0 + i + 1) << 8) | (unsigned long long)r.panel;
        else if (KEY == KEY_FIRST_ROW)
            key |= (unsigned long long)(n_total - (row0 + i));
        else
            key = (key | (r.srp == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(r.srp))) + 1ull;
        // The image only grows, so a dominated point needs no atomic.  The plain load races with other lanes' atomicMax on the same address:
        // an aligned 8-byte global load is one access (never torn), and a stale value is never larger than the current one, so the test can
        // only fail to skip, never skip wrongly.
        if (PRECHECK && img[at] >= key) continue;
        atomicMax(&img[at], key);
    }
}

struct PlotPaint {
    PlotDisc disc;
    PlotTicks ticks;
    int fixed;                 // fixed-colour mode
    uint32_t layer_rgb[2];
    double lo, hi;             // range of srp over the kept layer-1 rows
    int hline_py;              // -1: none
    uint32_t hline_rgb;
};

// ---- disc + colour pass: one thread per output pixel, the key image read through an LDS tile with a halo of D / 2 ------------------------------
// (one kernel: a second 8-byte image between the two steps would double the scratch memory)
template <class Src, int ORDERED>
__global__ void __launch_bounds__(256) k_plot_disc(const Src s, int64_t n, const PlotGeom G, const PlotPaint P, const unsigned long long *__restrict__ img,
                                                   uint8_t *__restrict__ rast) {
    extern __shared__ unsigned long long tile[];
    const int bx = blockIdx.x * PLOT_T, by = blockIdx.y * PLOT_T, panel = blockIdx.z;
    plot_tile_load(tile, img + (size_t)panel * G.H * G.W, G.W, G.H, bx, by, P.disc.h);
    __syncthreads();
    const int lx = threadIdx.x % PLOT_T;
    for (int ly = threadIdx.x / PLOT_T; ly < PLOT_T; ly += 256 / PLOT_T) {
        const int gx = bx + lx, gy = by + ly;
        if (gx >= G.W || gy >= G.H) continue;
        const unsigned long long m = plot_disc_max(tile, P.disc, lx, ly);
        uint32_t rgb;
        if (m == 0) {
            rgb = P.ticks.grid_or_background(gx, gy);
        } else {
            const int layer = (int)(m >> 63);
            const unsigned long long low = m & ~KEY_LAYER;
            if (P.fixed) {
                rgb = P.layer_rgb[layer];
            } else if (!layer) {
                rgb = PLOT_GREY;
            } else {
                double v;
                if (ORDERED) {
                    v = s.srp_at(n - (int64_t)low);
                    v = v == 0.0 ? 0.0 : v;
                } else {
                    v = __longlong_as_double((long long)(low - 1ull));
                }
                const double t = P.hi == P.lo ? 0.5 : (v - P.lo) / (P.hi - P.lo);
                rgb = plot_gradient(t);
            }
        }
        if (gy == P.hline_py) rgb = P.hline_rgb;
        plot_store_rgb(rast + (((size_t)panel * G.H + gy) * G.W + gx) * 3, rgb);
    }
}

// ---- heat map: nearest neighbour, row 0 at the bottom -------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_plot_heat(const double *__restrict__ htm, int B, int W, int H, const uint8_t *__restrict__ ramp, uint8_t *__restrict__ rast) {
    const int64_t total = (int64_t)W * H;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int px = (int)(i % W), py = (int)(i / W);
        const int r = (int)(((int64_t)(H - 1 - py) * B) / H), c = (int)(((int64_t)px * B) / W);
        const double v = htm[(size_t)r * B + c];
        int k = 0;
        if (isfinite(v)) {
            const double f = floor(v * (double)PLOT_RAMP_N);
            k = f >= (double)(PLOT_RAMP_N - 1) ? PLOT_RAMP_N - 1 : (f > 0.0 ? (int)f : 0);
        }
        rast[i * 3] = ramp[k * 3];
        rast[i * 3 + 1] = ramp[k * 3 + 1];
        rast[i * 3 + 2] = ramp[k * 3 + 2];
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------

// Device memory: ctx->plot_work (key image, rasters, partials) and ctx->plot_cols (host columns in chunks), the context's grow-only buffers.

// host columns (PlotFeed: x, y, srp, layer, panel): statistics pass, then centre pass, per chunk
using HostCols = PlotFeed<5>;
ColSrc chunk_src(const void *const *d) {
    return ColSrc{(const double *)d[0], (const double *)d[1], (const double *)d[2], (const uint8_t *)d[3], (const uint8_t *)d[4]};
}

struct PlotStats {
    double xr[2] = {0, 1}, yr[2] = {0, 1}, lo = NAN, hi = NAN;
    int64_t kept = 0, dropped = 0;
};

constexpr size_t PLOT_CONST_BYTES = (size_t)PLOT_MAX_BLOCKS * PLOT_NPART * 8 + 1024;   // statistics partials + the cluster marks
static_assert(PLOT_CONST_BYTES % 256 == 0, "the carved plot_work keeps its byte count");

int check_opts(const ldw_plot_opts *o, const char *who, int &D) {
    LDW_REQUIRE(o, LDW_ERR_ARG, "%s: null options", who);
    LDW_REQUIRE(o->kind >= LDW_PLOT_SR_CLUST && o->kind <= LDW_PLOT_LR, LDW_ERR_ARG, "%s: figure kind %d is no scatter figure", who, o->kind);
    D = o->D == 0 ? 11 : o->D;
    LDW_REQUIRE(D >= 1 && D <= LDW_PLOT_MAX_D && (D & 1), LDW_ERR_ARG, "%s: the disc diameter D = %d must be odd and in 1..%d", who, D, LDW_PLOT_MAX_D);
    LDW_REQUIRE(!o->has_hline || std::isfinite(o->hline_y), LDW_ERR_ARG, "%s: the line's y is not finite", who);
    return LDW_OK;
}

// one launch of the statistics pass over m rows, its partials merged into v
template <class Src>
int stats_accum(ldw_ctx *c, const Src &s, int64_t m, int n_panels, double *d_part, double *v) {
    const int grid = grid_for(m);
    LDW_LAUNCH(k_plot_stats<Src>, dim3(grid), dim3(256), 0, c->stream, s, m, n_panels, d_part);
    return plot_partials_merge<3, 4>(c, d_part, grid, v);
}

// one launch of the centre pass over rows row0 .. row0 + m - 1 of a table of n_total
template <class Src, int KEY>
void centre_launch(ldw_ctx *c, const Src &s, int64_t m, int64_t row0, int64_t n_total, int pre, const PlotGeom &G, unsigned long long *d_keys) {
    if (pre)
        hipLaunchKernelGGL((k_plot_centre<Src, KEY, 1>), dim3(grid_for(m)), dim3(256), 0, c->stream, s, m, row0, n_total, G, d_keys);
    else
        hipLaunchKernelGGL((k_plot_centre<Src, KEY, 0>), dim3(grid_for(m)), dim3(256), 0, c->stream, s, m, row0, n_total, G, d_keys);
}

// hc != NULL: the rows are host columns, fed in chunks (s is then only the colour pass's view)
template <class Src>
int plot_stats(ldw_ctx *c, const Src &s, const HostCols *hc, int64_t n, int n_panels, const ldw_plot_opts *o, double *d_part, PlotStats &st, const char *who) {
    if (n > 0) {
        double v[PLOT_NPART] = {INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY, 0, 0, 0, 0};
        if (hc) {
            if (int rc = hc->each_chunk(c, n, [&](const void *const *d, int64_t, int64_t m) { return stats_accum(c, chunk_src(d), m, n_panels, d_part, v); })) return rc;
        } else if (int rc = stats_accum(c, s, n, n_panels, d_part, v)) {
            return rc;
        }
        LDW_REQUIRE(v[8] == 0, LDW_ERR_ARG, "%s: a panel id lies outside 0..%d", who, n_panels - 1);
        st.kept = (int64_t)v[6];
        st.dropped = (int64_t)v[7];
        if (st.kept > 0) {
            st.xr[0] = v[0] == 0 ? 0.0 : v[0];
            st.xr[1] = v[1] == 0 ? 0.0 : v[1];
            st.yr[0] = v[2] == 0 ? 0.0 : v[2];
            st.yr[1] = v[3] == 0 ? 0.0 : v[3];
        }
        if (v[4] <= v[5]) {
            st.lo = v[4];
            st.hi = v[5];
        }
    }
    if (o->has_hline) {
        if (st.kept == 0) st.yr[0] = st.yr[1] = o->hline_y;
        st.yr[0] = std::min(st.yr[0], o->hline_y);
        st.yr[1] = std::max(st.yr[1], o->hline_y);
    }
    return LDW_OK;
}

// key image + rasters of n_panels panels of W x H pixels; ev (may be NULL): 4 events recorded after the clear, the centre pass, the disc pass
template <class Src>
int plot_raster(ldw_ctx *c, const Src &s, const HostCols *hc, bool has_srp, int64_t n, const ldw_plot_opts *o, int D, int n_panels, int W, int H, const double xlim[2], const double ylim[2],
                int nxt, const int32_t *xt, int nyt, const int32_t *yt, const PlotStats &st, unsigned long long *d_keys, uint8_t *d_rast, const Event *ev) {
    const PlotGeom G{xlim[0], xlim[1], ylim[0], ylim[1], W, H, n_panels};
    PlotPaint P{};
    P.disc = PlotDisc::make(D);
    P.ticks = PlotTicks::make(nxt, xt, nyt, yt);
    P.lo = st.lo;
    P.hi = st.hi;
    P.hline_py = o->has_hline ? H - 1 - plot_pixel(o->hline_y, ylim[0], ylim[1], H) : -1;
    P.hline_rgb = o->hline_rgb;
    P.layer_rgb[0] = o->layer_rgb[0];
    P.layer_rgb[1] = o->layer_rgb[1];
    P.fixed = has_srp ? 0 : 1;
    const size_t pixels = (size_t)n_panels * W * H;
    if (ev) LDW_HIP(hipEventRecord(ev[0], c->stream));
    LDW_HIP(hipMemsetAsync(d_keys, 0, pixels * 8, c->stream));
    if (ev) LDW_HIP(hipEventRecord(ev[1], c->stream));
    const int pre = (o->flags & LDW_PLOT_NO_PRECHECK) ? 0 : 1;
    const dim3 dgrid((W + PLOT_T - 1) / PLOT_T, (H + PLOT_T - 1) / PLOT_T, n_panels);
    auto run = [&](auto key_tag) -> int {
        constexpr int KEY = decltype(key_tag)::value;
        if (n > 0 && hc) {
            if (int rc = hc->each_chunk(c, n, [&](const void *const *d, int64_t i0, int64_t m) {
                    centre_launch<ColSrc, KEY>(c, chunk_src(d), m, i0, n, pre, G, d_keys);
                    return (int)LDW_OK;
                }))
                return rc;
        } else if (n > 0) {
            centre_launch<Src, KEY>(c, s, n, 0, n, pre, G, d_keys);
        }
        if (ev) LDW_HIP(hipEventRecord(ev[2], c->stream));
        hipLaunchKernelGGL((k_plot_disc<Src, KEY == KEY_FIRST_ROW>), dgrid, dim3(256), plot_tile_lds(P.disc), c->stream, s, n, G, P, d_keys, d_rast);
        if (ev) LDW_HIP(hipEventRecord(ev[3], c->stream));
        LDW_HIP(hipGetLastError());
        return LDW_OK;
    };
    return o->ordered ? run(std::integral_constant<int, KEY_FIRST_ROW>()) : run(std::integral_constant<int, KEY_SRP>());
}

template <class Src>
int plot_panels(ldw_ctx *c, const Src &s, const HostCols *hc, bool has_srp, int64_t n, const ldw_plot_opts *o, int n_panels, int W, int H, uint8_t *rgb_out, double *stats_out,
                int64_t *scratch_out, double *ms_out, const char *who) {
    int D = 0;
    if (int rc = check_opts(o, who, D)) return rc;
    LDW_REQUIRE(!o->ordered || has_srp || n == 0, LDW_ERR_ARG, "%s: the row-order key needs the srp column", who);
    LDW_REQUIRE(n_panels >= 1 && n_panels <= LDW_PLOT_MAX_PANELS, LDW_ERR_ARG, "%s: %d panels outside 1..%d", who, n_panels, LDW_PLOT_MAX_PANELS);
    LDW_REQUIRE(W >= 1 && H >= 1 && (int64_t)W * H * n_panels <= (1ll << 28), LDW_ERR_ARG, "%s: panels of %d x %d pixels", who, W, H);
    LDW_REQUIRE(rgb_out, LDW_ERR_ARG, "%s: null output", who);
    const size_t pixels = (size_t)n_panels * W * H;
    Carve cv;
    auto d_keys = cv.take<unsigned long long>((int64_t)pixels);
    auto d_rast = cv.take<uint8_t>((int64_t)pixels * 3);
    auto d_part = cv.take<double>(PLOT_CONST_BYTES / 8);
    if (int rc = cv.reserve(c->plot_work)) return rc;
    if (scratch_out) *scratch_out = (int64_t)cv.bytes;
    PlotEvents<2> ev_stats;   // round the statistics pass
    PlotEvents<4> ev;         // round the clear, the centre pass, the disc pass
    if (ms_out) {
        LDW_HIP(ev_stats.create());
        LDW_HIP(ev.create());
    }
    PlotStats st;
    if (ms_out) LDW_HIP(hipEventRecord(ev_stats.e[0], c->stream));
    if (int rc = plot_stats(c, s, hc, n, n_panels, o, d_part, st, who)) return rc;
    if (ms_out) LDW_HIP(hipEventRecord(ev_stats.e[1], c->stream));
    double xlim[2], ylim[2], tick[LDW_PLOT_MAX_TICKS];
    int32_t xt[LDW_PLOT_MAX_TICKS], yt[LDW_PLOT_MAX_TICKS], nxt = 0, nyt = 0;
    LDW_REQUIRE(plot_axis(st.xr[0], st.xr[1], W, 0, xlim, tick, xt, &nxt) == LDW_OK && plot_axis(st.yr[0], st.yr[1], H, 1, ylim, tick, yt, &nyt) == LDW_OK,
                LDW_ERR_ARG, "%s: the data ranges are not finite intervals", who);
    if (int rc = plot_raster(c, s, hc, has_srp, n, o, D, n_panels, W, H, xlim, ylim, nxt, xt, nyt, yt, st, d_keys, d_rast, ms_out ? ev.e : nullptr)) return rc;
    LDW_HIP(hipMemcpyAsync(rgb_out, d_rast, pixels * 3, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    if (ms_out) {
        LDW_HIP(ev_stats.elapsed(ms_out));
        LDW_HIP(ev.elapsed(ms_out + 1));
    }
    if (stats_out) {
        const double v[8] = {st.xr[0], st.xr[1], st.yr[0], st.yr[1], st.lo, st.hi, (double)st.kept, (double)st.dropped};
        memcpy(stats_out, v, sizeof(v));
    }
    return LDW_OK;
}

int emit_figure(const ldw_plot_layout &lay, int kind, const std::vector<uint8_t> &rasters, const int32_t *panel_label, const char *title, bool cb_valid,
                double cb_lo, double cb_hi, const char *png_path, uint8_t *rgb_out) {
    PlotCanvas canvas(rgb_out, lay.width, lay.height);
    plot_frame(canvas.rgb, lay, kind, rasters.data(), panel_label, title, cb_valid, cb_lo, cb_hi);
    return canvas.finish(png_path);
}

// the whole figure: statistics -> layout -> rasters -> frame -> PNG / canvas
template <class Src>
int plot_figure(ldw_ctx *c, const Src &s, const HostCols *hc, bool has_srp, int64_t n, const ldw_plot_opts *o, int n_panels, const int32_t *panel_label, const char *png_path,
                uint8_t *rgb_out, int64_t *dropped_out, const char *who) {
    int D = 0;
    if (int rc = check_opts(o, who, D)) return rc;
    LDW_REQUIRE(!o->ordered || has_srp || n == 0, LDW_ERR_ARG, "%s: the row-order key needs the srp column", who);
    LDW_REQUIRE(n_panels >= 1 && n_panels <= LDW_PLOT_MAX_PANELS && (o->kind == LDW_PLOT_SR_CLUST || n_panels == 1), LDW_ERR_ARG,
                "%s: %d panels (1..%d for the facet figure, 1 otherwise)", who, n_panels, LDW_PLOT_MAX_PANELS);
    LDW_REQUIRE(png_path || rgb_out, LDW_ERR_ARG, "%s: neither a path nor a canvas to write to", who);
    ldw_plot_layout lay;
    if (int rc = ldw_plot_layout_get(o->kind, n_panels, 0, 1, 0, 1, &lay)) return rc;   // (panel size: independent of the ranges)
    const int W = lay.panel_w, H = lay.panel_h;
    const size_t pixels = (size_t)n_panels * W * H;
    Carve cv;
    auto d_keys = cv.take<unsigned long long>((int64_t)pixels);
    auto d_rast = cv.take<uint8_t>((int64_t)pixels * 3);
    auto d_part = cv.take<double>(PLOT_CONST_BYTES / 8);
    if (int rc = cv.reserve(c->plot_work)) return rc;
    PlotStats st;
    if (int rc = plot_stats(c, s, hc, n, n_panels, o, d_part, st, who)) return rc;
    if (int rc = ldw_plot_layout_get(o->kind, n_panels, st.xr[0], st.xr[1], st.yr[0], st.yr[1], &lay)) return rc;
    if (int rc = plot_raster(c, s, hc, has_srp, n, o, D, n_panels, W, H, lay.xlim, lay.ylim, lay.n_xticks, lay.xtick_px, lay.n_yticks, lay.ytick_px, st,
                             d_keys, d_rast, nullptr))
        return rc;
    std::vector<uint8_t> rasters(pixels * 3);
    LDW_HIP(hipMemcpyAsync(rasters.data(), d_rast, pixels * 3, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    if (dropped_out) *dropped_out = st.dropped;
    return emit_figure(lay, o->kind, rasters, panel_label, nullptr, has_srp && st.lo <= st.hi, st.lo, st.hi, png_path, rgb_out);
}

// The caller's columns as the passes see them.  Device columns: read where they lie.  Host columns: fed in chunks (HostCols), so the device holds
// one chunk at a time — and, for the row-order key alone, the whole srp column (8 B per row), which the colour pass reads by row.
struct Cols {
    ColSrc src{};
    HostCols host{};
    const HostCols *hc = nullptr;
    int make(ldw_ctx *c, const double *x, const double *y, const double *srp, const uint8_t *layer, const uint8_t *panel, int64_t n, int on_device,
             int ordered) {
        src = ColSrc{x, y, srp, layer, panel};
        if (on_device || n == 0) return LDW_OK;
        host = HostCols{{x, y, srp, layer, panel}, {8, 8, 8, 1, 1}};
        hc = &host;
        const size_t cb = host.chunk_bytes(n);
        const bool whole_srp = ordered && srp;
        if (int rc = c->plot_cols.reserve(cb + (whole_srp ? (size_t)n * 8 : 0))) return rc;
        src = ColSrc{nullptr, nullptr, nullptr, nullptr, nullptr};
        if (whole_srp) {
            double *d = (double *)(c->plot_cols.as<uint8_t>() + cb);
            LDW_HIP(hipMemcpyAsync(d, srp, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
            src.srp = d;
        }
        return LDW_OK;
    }
};

int check_cols(const double *x, const double *y, int64_t n, const char *who) {
    LDW_REQUIRE(n >= 0, LDW_ERR_ARG, "%s: n = %lld < 0", who, (long long)n);
    LDW_REQUIRE(n == 0 || (x && y), LDW_ERR_ARG, "%s: null x or y column", who);
    return LDW_OK;
}

int heat_figure(ldw_ctx *c, const double *d_htm, int32_t B, const char *title, const char *png_path, uint8_t *rgb_out) {
    ldw_plot_layout lay;
    if (int rc = ldw_plot_layout_get(LDW_PLOT_LDMAP, 1, 0, 1, 0, 1, &lay)) return rc;
    const int W = lay.panel_w, H = lay.panel_h;
    const size_t pixels = (size_t)W * H;
    if (int rc = c->plot_work.reserve(round256(pixels * 3) + PLOT_RAMP_N * 3)) return rc;
    uint8_t *d_rast = c->plot_work.as<uint8_t>(), *d_ramp = d_rast + round256(pixels * 3);
    std::vector<uint8_t> ramp(PLOT_RAMP_N * 3);
    plot_ramp_table(ramp.data());
    LDW_HIP(hipMemcpyAsync(d_ramp, ramp.data(), ramp.size(), hipMemcpyHostToDevice, c->stream));
    LDW_LAUNCH(k_plot_heat, dim3(2048), dim3(256), 0, c->stream, d_htm, (int)B, W, H, d_ramp, d_rast);
    std::vector<uint8_t> rasters(pixels * 3);
    LDW_HIP(hipMemcpyAsync(rasters.data(), d_rast, pixels * 3, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    return emit_figure(lay, LDW_PLOT_LDMAP, rasters, nullptr, title, false, 0, 0, png_path, rgb_out);
}

}  // namespace

int plot_stats_accum(ldw_ctx *c, const ColSrc &s, int64_t m, int n_panels, double *d_part, double *v) { return stats_accum(c, s, m, n_panels, d_part, v); }

int plot_centre_classes(ldw_ctx *c, const ColSrc &s, int64_t m, int64_t row0, const PlotGeom &G, unsigned long long *d_keys) {
    LDW_LAUNCH((k_plot_centre<ColSrc, KEY_CLASS, 1>), dim3(grid_for(m)), dim3(256), 0, c->stream, s, m, row0, (int64_t)0, G, d_keys);
    return LDW_OK;
}

}  // namespace ldw

using namespace ldw;

extern "C" {

int ldw_plot_scatter(ldw_ctx *c, const double *x, const double *y, const double *srp, const uint8_t *layer, const uint8_t *panel, int64_t n, int on_device,
                     const ldw_plot_opts *opts, int n_panels, const int32_t *panel_label, const char *png_path, uint8_t *rgb_out, int64_t *dropped_out) {
    LDW_REQUIRE(c != nullptr, LDW_ERR_ARG, "ldw_plot_scatter: null context");
    if (int rc = check_cols(x, y, n, "ldw_plot_scatter")) return rc;
    int D = 0;
    if (int rc = check_opts(opts, "ldw_plot_scatter", D)) return rc;
    LDW_REQUIRE(n_panels >= 1 && n_panels <= LDW_PLOT_MAX_PANELS && (opts->kind == LDW_PLOT_SR_CLUST || n_panels == 1), LDW_ERR_ARG,
                "ldw_plot_scatter: %d panels (1..%d for the facet figure, 1 otherwise)", n_panels, LDW_PLOT_MAX_PANELS);
    LDW_REQUIRE(png_path || rgb_out, LDW_ERR_ARG, "ldw_plot_scatter: neither a path nor a canvas to write to");
    if (int rc = check_gpu(c)) return rc;
    Cols cols;
    if (int rc = cols.make(c, x, y, srp, layer, panel, n, on_device, opts->ordered)) return rc;
    return plot_figure(c, cols.src, cols.hc, srp != nullptr, n, opts, n_panels, panel_label, png_path, rgb_out, dropped_out, "ldw_plot_scatter");
}

int ldw_debug_plot_panels(ldw_ctx *c, const double *x, const double *y, const double *srp, const uint8_t *layer, const uint8_t *panel, int64_t n, int on_device,
                          const ldw_plot_opts *opts, int n_panels, int32_t W, int32_t H, uint8_t *rgb_out, double *stats_out, int64_t *scratch_bytes_out,
                          double *ms_out) {
    LDW_REQUIRE(c != nullptr, LDW_ERR_ARG, "ldw_debug_plot_panels: null context");
    if (int rc = check_cols(x, y, n, "ldw_debug_plot_panels")) return rc;
    int D = 0;
    if (int rc = check_opts(opts, "ldw_debug_plot_panels", D)) return rc;
    if (int rc = check_gpu(c)) return rc;
    Cols cols;
    if (int rc = cols.make(c, x, y, srp, layer, panel, n, on_device, opts->ordered)) return rc;
    return plot_panels(c, cols.src, cols.hc, srp != nullptr, n, opts, n_panels, W, H, rgb_out, stats_out, scratch_bytes_out, ms_out, "ldw_debug_plot_panels");
}

int ldw_plot_links(ldw_ctx *c, int which, int use_aracne, const ldw_plot_opts *opts, const char *png_path, uint8_t *rgb_out, int64_t *dropped_out) {
    LDW_REQUIRE(c != nullptr, LDW_ERR_ARG, "ldw_plot_links: null context");
    LDW_REQUIRE(which == 0 || which == 1, LDW_ERR_ARG, "ldw_plot_links: which = %d (0 short-range, 1 long-range)", which);
    int D = 0;
    if (int rc = check_opts(opts, "ldw_plot_links", D)) return rc;
    LDW_REQUIRE(which == 0 ? opts->kind != LDW_PLOT_LR : opts->kind == LDW_PLOT_LR, LDW_ERR_ARG, "ldw_plot_links: figure kind %d does not fit table %d",
                opts->kind, which);
    LDW_REQUIRE(png_path || rgb_out, LDW_ERR_ARG, "ldw_plot_links: neither a path nor a canvas to write to");
    if (int rc = check_gpu(c)) return rc;
    LDW_REQUIRE(c->meta.POS.p != nullptr, LDW_ERR_STATE, "ldw_plot_links: no SNP meta data (ldw_set_snp_meta)");
    LDW_REQUIRE(c->meta.g > 0, LDW_ERR_STATE, "ldw_plot_links: the genome length is not known (ldw_set_positions with g = 0): len cannot be taken from the positions");
    LDW_REQUIRE((which == 1) == c->kept.from_lr, LDW_ERR_STATE, "ldw_plot_links: the kept links are those of the %s table", c->kept.from_lr ? "long-range" : "short-range");
    const int64_t n = c->kept.n_red;
    LDW_REQUIRE(!use_aracne || n == 0 || (c->kept.ar_valid && c->kept.ar_flags.cap >= (size_t)n), LDW_ERR_STATE,
                "ldw_plot_links: ldw_aracne_device has not run for the kept links (use_aracne = 0 draws every link as direct)");
    CtxSrc s;
    memset(&s, 0, sizeof(s));
    s.row = c->kept.row.as<int64_t>();
    s.a = (which ? c->links.lr_a : c->links.sr_a).as<int32_t>();
    s.b = (which ? c->links.lr_b : c->links.sr_b).as<int32_t>();
    s.mi = (which ? c->links.lr_mi : c->links.sr_mi).as<double>();
    s.POS = c->meta.POS.as<int32_t>();
    s.g = c->meta.g;
    s.srp = which ? nullptr : c->kept.srp.as<double>();
    s.meta = which ? nullptr : c->kept.meta.as<uint32_t>();
    s.flags = use_aracne && n > 0 ? c->kept.ar_flags.as<uint8_t>() : nullptr;
    int n_panels = 1;
    int32_t labels[LDW_PLOT_MAX_PANELS] = {1};
    if (opts->kind == LDW_PLOT_SR_CLUST && n > 0) {
        // the facets: the clust_c values present, ascending
        if (int rc = c->plot_work.reserve(1024)) return rc;
        void *marks = c->plot_work.p;
        LDW_HIP(hipMemsetAsync(marks, 0, 1024, c->stream));
        LDW_LAUNCH(k_plot_present, dim3(grid_for(n)), dim3(256), 0, c->stream, s.meta, n, (uint32_t *)marks);
        uint32_t present[256];
        LDW_HIP(hipMemcpyAsync(present, marks, 1024, hipMemcpyDeviceToHost, c->stream));
        LDW_HIP(hipStreamSynchronize(c->stream));
        n_panels = 0;
        for (int k = 0; k < 256; ++k)
            if (present[k]) {
                LDW_REQUIRE(n_panels < LDW_PLOT_MAX_PANELS, LDW_ERR_ARG, "ldw_plot_links: more than %d clusters hold links", LDW_PLOT_MAX_PANELS);
                s.lut[k] = (uint8_t)n_panels;
                labels[n_panels++] = k;
            }
        s.facets = 1;
    }
    return plot_figure(c, s, nullptr, s.srp != nullptr, n, opts, n_panels, labels, png_path, rgb_out, dropped_out, "ldw_plot_links");
}

int ldw_plot_heatmap(ldw_ctx *c, const double *htm, int32_t B, int on_device, const char *title, const char *png_path, uint8_t *rgb_out) {
    LDW_REQUIRE(c != nullptr, LDW_ERR_ARG, "ldw_plot_heatmap: null context");
    LDW_REQUIRE(htm && B >= 1 && B <= 32768, LDW_ERR_ARG, "ldw_plot_heatmap: null map or B = %d outside 1..32768", B);
    LDW_REQUIRE(png_path || rgb_out, LDW_ERR_ARG, "ldw_plot_heatmap: neither a path nor a canvas to write to");
    if (int rc = check_gpu(c)) return rc;
    const double *d = htm;
    if (!on_device) {
        if (int rc = c->plot_cols.reserve((size_t)B * B * 8)) return rc;
        LDW_HIP(hipMemcpyAsync(c->plot_cols.p, htm, (size_t)B * B * 8, hipMemcpyHostToDevice, c->stream));
        d = c->plot_cols.as<double>();
    }
    return heat_figure(c, d, B, title, png_path, rgb_out);
}

int ldw_plot_ldmap(ldw_ctx *c, int32_t reducer, int32_t from, int32_t to, const char *title, const char *png_path, int64_t *n_pos_out, int32_t *reducer_out,
                   int32_t *B_out, double *htm_out, int64_t capacity) {
    LDW_REQUIRE(c != nullptr, LDW_ERR_ARG, "ldw_plot_ldmap: null context");
    LDW_REQUIRE(png_path, LDW_ERR_ARG, "ldw_plot_ldmap: null path");
    const double *d_htm = nullptr;
    if (int rc = ldmap_device(c, reducer, from, to, n_pos_out, reducer_out, B_out, true, htm_out ? capacity : -1, &d_htm)) return rc;
    const int32_t B = *B_out;
    if (htm_out) LDW_HIP(hipMemcpyAsync(htm_out, d_htm, (size_t)B * B * 8, hipMemcpyDeviceToHost, c->stream));
    return heat_figure(c, d_htm, B, title, png_path, nullptr);
}

}  // extern "C"
