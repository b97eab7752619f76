// The raster primitives under the figure renderers (ldw_plot*.hip; DESIGN.md 20 "The shared pieces"): every rule a second renderer needs is
// stated here once.  Device pieces are built into each kernel that uses them; two kernels that do different work stay two kernels.
#pragma once
#include <algorithm>
#include <vector>

#include "ldw_dev.h"
#include "ldw_work.h"
#include "ldw_plot.h"

namespace ldw {

constexpr int PLOT_T = 32;                    // the tile of the disc, paint and shade passes: PLOT_T x PLOT_T pixels per block of 256 threads
constexpr int PLOT_NPART = 10, PLOT_MAX_BLOCKS = 1024;
constexpr int64_t PLOT_CHUNK = 1 << 20;       // rows of host columns per upload (26 MiB of the scatter's five columns)
constexpr int PLOT_COORD_LO = -8192, PLOT_COORD_HI = 16383;   // the window of a mark's coordinates: keeps the coverage products below 2^62

inline size_t round256(size_t b) { return (b + 255) & ~(size_t)255; }
inline int grid_for(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, PLOT_MAX_BLOCKS)); }

__device__ __forceinline__ void plot_store_rgb(uint8_t *o, uint32_t rgb) {
    o[0] = (uint8_t)(rgb >> 16);
    o[1] = (uint8_t)(rgb >> 8);
    o[2] = (uint8_t)rgb;
}

// ---- the point's disc and the panel's grid lines ------------------------------------------------------------------------------------------------
struct PlotDisc {
    int D, h;                    // diameter, halo = D / 2
    int8_t hw[LDW_PLOT_MAX_D];   // hw[dy + h] = largest dx with 4 (dx^2 + dy^2) <= D^2
    static PlotDisc make(int D) {
        PlotDisc d{};
        d.D = D;
        d.h = D / 2;
        for (int dy = -d.h; dy <= d.h; ++dy) {
            int w = 0;
            while (4 * ((w + 1) * (w + 1) + dy * dy) <= D * D) ++w;
            d.hw[dy + d.h] = (int8_t)w;
        }
        return d;
    }
};

struct PlotTicks {
    int nx, ny, xt[LDW_PLOT_MAX_TICKS], yt[LDW_PLOT_MAX_TICKS];   // panel pixels of the grid lines
    static PlotTicks make(int nx, const int32_t *xt, int ny, const int32_t *yt) {
        PlotTicks t{};
        t.nx = nx;
        t.ny = ny;
        std::copy(xt, xt + nx, t.xt);
        std::copy(yt, yt + ny, t.yt);
        return t;
    }
    __device__ __forceinline__ uint32_t grid_or_background(int gx, int gy) const {
        bool grid = false;
        for (int k = 0; k < nx; ++k) grid |= xt[k] == gx;
        for (int k = 0; k < ny; ++k) grid |= yt[k] == gy;
        return grid ? PLOT_GRID : PLOT_BG;
    }
};

inline size_t plot_tile_lds(const PlotDisc &d) { return (size_t)(PLOT_T + 2 * d.h) * (PLOT_T + 2 * d.h) * 8; }

// the key image round the tile at (bx, by), with a halo of h pixels, into tile[(PLOT_T + 2 h)^2]; the caller synchronises before it reads
__device__ __forceinline__ void plot_tile_load(unsigned long long *tile, const unsigned long long *__restrict__ img, int W, int H, int bx, int by, int h) {
    const int tw = PLOT_T + 2 * h;
    for (int t = threadIdx.x; t < tw * tw; t += 256) {
        const int gx = bx - h + t % tw, gy = by - h + t / tw;
        tile[t] = (gx >= 0 && gx < W && gy >= 0 && gy < H) ? img[(size_t)gy * W + gx] : 0ull;   // discs are clipped at the panel
    }
}

// the maximum of the loaded tile over the disc round the tile's pixel (lx, ly)
__device__ __forceinline__ unsigned long long plot_disc_max(const unsigned long long *tile, const PlotDisc &d, int lx, int ly) {
    const int h = d.h, tw = PLOT_T + 2 * h;
    unsigned long long m = 0;
    for (int dy = -h; dy <= h; ++dy) {
        const int w = d.hw[dy + h];
        const unsigned long long *rowp = tile + (ly + h + dy) * tw + lx + h;
        for (int dx = -w; dx <= w; ++dx) m = max(m, rowp[dx]);
    }
    return m;
}

// ---- partials of a statistics pass: v[0 .. 2 PAIRS) are (min, max) pairs, the SUMS entries behind them sums (counts below 2^53: exact) ----------
template <int PAIRS, int SUMS> __host__ __device__ __forceinline__ double plot_partial_join(int k, double p, double q) {
    return k >= 2 * PAIRS ? p + q : ((k & 1) ? fmax(p, q) : fmin(p, q));
}

// a block of 256 threads: the block's partials into part[blockIdx.x][2 PAIRS + SUMS]
template <int PAIRS, int SUMS> __device__ __forceinline__ void plot_partials_reduce(const double *v, double *__restrict__ part) {
    constexpr int N = 2 * PAIRS + SUMS;
    __shared__ double sh[256];
    for (int k = 0; k < N; ++k) {
        sh[threadIdx.x] = v[k];
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) sh[threadIdx.x] = plot_partial_join<PAIRS, SUMS>(k, sh[threadIdx.x], sh[threadIdx.x + w]);
            __syncthreads();
        }
        if (threadIdx.x == 0) part[(size_t)blockIdx.x * N + k] = sh[0];
        __syncthreads();
    }
}

// the partials of grid blocks, read back over the context's stream, merged into v
template <int PAIRS, int SUMS> int plot_partials_merge(ldw_ctx *c, const double *d_part, int grid, double *v) {
    constexpr int N = 2 * PAIRS + SUMS;
    std::vector<double> part((size_t)grid * N);
    LDW_HIP(hipMemcpyAsync(part.data(), d_part, part.size() * 8, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    for (int b = 0; b < grid; ++b)
        for (int k = 0; k < N; ++k) v[k] = plot_partial_join<PAIRS, SUMS>(k, v[k], part[(size_t)b * N + k]);
    return LDW_OK;
}

// ---- a capsule — the segment from end 0 to end 1 with a width w, w2 = w^2 — covers the pixel (x, y) iff 4 D2 <= w2 --------------------------------
// With p = pixel - end 0 and d = end 1 - end 0, the squared distance D2 from the pixel to the segment is |p|^2 where p.d <= 0, |p - d|^2 where
// p.d >= |d|^2, and (p x d)^2 / |d|^2 between: evaluated in int64 as 4 (p x d)^2 <= w2 |d|^2 there.  Coordinates inside the window and w <= 1024
// keep |p x d| < 2^30 and every product below 2^62.
__host__ __device__ __forceinline__ bool plot_capsule_covers(int x0, int y0, int x1, int y1, int64_t w2, int x, int y) {
    const int64_t px = x - x0, py = y - y0, dx = x1 - x0, dy = y1 - y0;
    const int64_t dd = dx * dx + dy * dy, t = px * dx + py * dy;
    if (t <= 0) return 4 * (px * px + py * py) <= w2;
    if (t >= dd) {
        const int64_t qx = px - dx, qy = py - dy;
        return 4 * (qx * qx + qy * qy) <= w2;
    }
    const int64_t cr = px * dy - py * dx;
    return 4 * cr * cr <= w2 * dd;
}

// mark i of a list (a capsule, a rectangle: x0, y0, x1, y1) lies inside the coordinate window
template <class Mark> int plot_check_window(const Mark &m, long long i, const char *what, const char *who) {
    const int lo = std::min(std::min(m.x0, m.y0), std::min(m.x1, m.y1)), hi = std::max(std::max(m.x0, m.y0), std::max(m.x1, m.y1));
    LDW_REQUIRE(lo >= PLOT_COORD_LO && hi <= PLOT_COORD_HI, LDW_ERR_ARG, "%s: %s %lld has a coordinate outside %d..%d", who, what, i, PLOT_COORD_LO, PLOT_COORD_HI);
    return LDW_OK;
}

// ---- host columns travel in chunks of PLOT_CHUNK rows through ctx->plot_cols, a device buffer of constant size --------------------------------------
// Column k of a chunk lies behind the slots (rounded to 256 bytes) of the columns before it, given or not.
template <int N> struct PlotFeed {
    const void *col[N];   // host; NULL: not given
    int elem[N];          // bytes per row
    size_t chunk_bytes(int64_t n) const {
        size_t b = 0;
        for (int k = 0; k < N; ++k) b += round256((size_t)std::min<int64_t>(n, PLOT_CHUNK) * elem[k]);
        return b;
    }
    // rows [i0, i0 + m) of a table of n into the buffer (reserved by the caller), queued on the context's stream behind the kernels that read the
    // last chunk; dev[k]: where column k lies, NULL if not given
    int upload(ldw_ctx *c, int64_t n, int64_t i0, int64_t m, const void *dev[N]) const {
        uint8_t *p = c->plot_cols.as<uint8_t>();
        for (int k = 0; k < N; ++k) {
            dev[k] = col[k] ? p : nullptr;
            if (col[k]) LDW_HIP(hipMemcpyAsync(p, (const uint8_t *)col[k] + (size_t)i0 * elem[k], (size_t)m * elem[k], hipMemcpyHostToDevice, c->stream));
            p += round256((size_t)std::min<int64_t>(n, PLOT_CHUNK) * elem[k]);
        }
        return LDW_OK;
    }
    // f(dev, i0, m) for every chunk of the table
    template <class F> int each_chunk(ldw_ctx *c, int64_t n, F f) const {
        for (int64_t i0 = 0; i0 < n; i0 += PLOT_CHUNK) {
            const int64_t m = std::min<int64_t>(PLOT_CHUNK, n - i0);
            const void *dev[N];
            if (int rc = upload(c, n, i0, m, dev)) return rc;
            if (int rc = f(dev, i0, m)) return rc;
        }
        return LDW_OK;
    }
};

// ---- the scatter's rows, and the two passes over them that the xy figures share (ldw_plot.hip) -------------------------------------------------------
struct PlotRow {
    double x, y, srp;
    int layer, panel;
};

// the caller's columns on the device.  The xy figures put the class into the panel slot and give neither srp nor layer.
struct ColSrc {
    const double *x, *y, *srp;
    const uint8_t *layer, *panel;
    __device__ __forceinline__ bool has_srp() const { return srp != nullptr; }
    __device__ __forceinline__ double srp_at(int64_t i) const { return srp[i]; }
    __device__ __forceinline__ void get(int64_t i, PlotRow &r) const {
        r.x = x[i];
        r.y = y[i];
        r.srp = srp ? srp[i] : 0.0;
        r.layer = layer ? (layer[i] != 0) : 1;
        r.panel = panel ? panel[i] : 0;
    }
};

struct PlotGeom {
    double x0, x1, y0, y1;
    int W, H, n_panels;   // (the xy figures: one panel, n_panels = the number of classes)
};

// One launch of the statistics pass over m device rows, its partials merged into v[PLOT_NPART]: (min, max) of x, y and of srp over the layer-1
// rows, taken over the kept rows; rows kept; rows dropped; non-zero if a row's panel lies outside 0..n_panels - 1.  d_part: PLOT_MAX_BLOCKS x PLOT_NPART.
int plot_stats_accum(ldw_ctx *c, const ColSrc &s, int64_t m, int n_panels, double *d_part, double *v);
// one launch of the centre pass in the xy figures' key order over rows row0 .. row0 + m - 1: key (row + 1) << 8 | class, the LAST row on top
int plot_centre_classes(ldw_ctx *c, const ColSrc &s, int64_t m, int64_t row0, const PlotGeom &G, unsigned long long *d_keys);

// ---- the caller's canvas[H][W][3] or one of our own, and the PNG at the end ------------------------------------------------------------------------
struct PlotCanvas {
    std::vector<uint8_t> own;
    uint8_t *rgb;
    int W, H;
    PlotCanvas(uint8_t *rgb_out, int W_, int H_) : rgb(rgb_out), W(W_), H(H_) {
        if (!rgb) {
            own.resize((size_t)W * H * 3);
            rgb = own.data();
        }
    }
    int finish(const char *png_path) const { return png_path ? ldw_png_write(png_path, rgb, W, H, -1, nullptr) : LDW_OK; }
};

}  // namespace ldw
