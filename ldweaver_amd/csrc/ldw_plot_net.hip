// The edges of the network plot on the device (include/ldweaver_amd.h 12): translucent capsules — a segment with a width — blended
// in list order over a white canvas.
//
// Rule.  The endpoints and the pixels are integer points (the centre of pixel (x, y) is the point (x, y)); a pixel is covered iff its squared
// distance D2 to the segment satisfies 4 D2 <= w^2 (plot_capsule_covers, ldw_plot_prim.h: exact in int64 for coordinates inside the window and
// w <= NET_MAX_W).  A covered pixel takes c = (c (255 - a) + col a + 127) / 255 per channel.
//
// Kernels.  k_net_boxes: the tiles (32 x 32 pixels) that a capsule's bounding box, inflated by ceil(w / 2) and clipped at the canvas, meets.
// k_net_bin: one thread per tile walks the boxes IN LIST ORDER (staged through LDS 256 at a time), first counting, then — behind rocPRIM's exclusive
// sum — writing the indices of the capsules that meet its tile: the tile's list is in draw order by construction, no atomics and no sort.
// k_net_shade: one block per tile, one thread per pixel (four rows each), every pixel walks its tile's list.
//
// Bounds: a tile's list entries lie in [off[tile], off[tile + 1]) of a list of off[tiles] entries; a pixel is written only inside the canvas.
#include <algorithm>
#include <vector>

#include "ldw_plot_prim.h"

namespace ldw {
namespace {

constexpr int NET_T = PLOT_T;
constexpr int NET_MAX_DIM = 8192, NET_MAX_W = 1024;
constexpr int64_t NET_MAX_CAPS = 1 << 17;   // k_net_bin tests every capsule against every tile, twice: 8192 edges of 16 segments is what that serves

struct TileBox {
    int16_t tx0, ty0, tx1, ty1;   // tiles tx0..tx1 x ty0..ty1; tx0 > tx1: none
};

__global__ __launch_bounds__(256) void k_net_boxes(const ldw_capsule *__restrict__ caps, int64_t n, int W, int H, TileBox *__restrict__ box) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const ldw_capsule c = caps[i];
    const int h = (c.w + 1) / 2;
    const int xa = max(min(c.x0, c.x1) - h, 0), xb = min(max(c.x0, c.x1) + h, W - 1);
    const int ya = max(min(c.y0, c.y1) - h, 0), yb = min(max(c.y0, c.y1) + h, H - 1);
    TileBox b;
    if (xa > xb || ya > yb) {
        b.tx0 = 1;
        b.tx1 = 0;
        b.ty0 = 1;
        b.ty1 = 0;
    } else {
        b.tx0 = (int16_t)(xa / NET_T);
        b.tx1 = (int16_t)(xb / NET_T);
        b.ty0 = (int16_t)(ya / NET_T);
        b.ty1 = (int16_t)(yb / NET_T);
    }
    box[i] = b;
}

// FILL = 0: cnt[tile] = capsules whose box meets the tile.  FILL = 1: list[off[tile] ..] = their indices, ascending.
template <int FILL>
__global__ __launch_bounds__(256) void k_net_bin(const TileBox *__restrict__ box, int64_t n, int ntx, int ntiles, uint32_t *__restrict__ cnt, const uint32_t *__restrict__ off,
                                                 uint32_t *__restrict__ list) {
    __shared__ TileBox sh[256];
    const int tile = blockIdx.x * 256 + threadIdx.x;
    const int tx = tile % ntx, ty = tile / ntx;
    uint32_t k = (FILL && tile < ntiles) ? off[tile] : 0;
    for (int64_t base = 0; base < n; base += 256) {
        __syncthreads();
        if (base + threadIdx.x < n) sh[threadIdx.x] = box[base + threadIdx.x];
        __syncthreads();
        const int m = (int)min((int64_t)256, n - base);
        if (tile < ntiles)
            for (int j = 0; j < m; ++j) {
                const TileBox b = sh[j];
                if (tx >= b.tx0 && tx <= b.tx1 && ty >= b.ty0 && ty <= b.ty1) {
                    if (FILL) list[k] = (uint32_t)(base + j);
                    ++k;
                }
            }
    }
    if (!FILL && tile < ntiles) cnt[tile] = k;
}

__global__ __launch_bounds__(256) void k_net_shade(const ldw_capsule *__restrict__ caps, const uint32_t *__restrict__ off, const uint32_t *__restrict__ list, int W, int H,
                                                   uint8_t *__restrict__ rast) {
    const int tile = blockIdx.y * gridDim.x + blockIdx.x;
    const uint32_t lo = off[tile], hi = off[tile + 1];
    const int x = blockIdx.x * NET_T + (threadIdx.x % NET_T);
    const int y0 = blockIdx.y * NET_T + (threadIdx.x / NET_T);
    int r[4], g[4], b[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) r[q] = g[q] = b[q] = 255;
    for (uint32_t k = lo; k < hi; ++k) {
        const ldw_capsule c = caps[list[k]];
        const int cr = (int)(c.rgb >> 16 & 0xff), cg = (int)(c.rgb >> 8 & 0xff), cb = (int)(c.rgb & 0xff), a = c.alpha;
        const int64_t w2 = (int64_t)c.w * c.w;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (plot_capsule_covers(c.x0, c.y0, c.x1, c.y1, w2, x, y0 + 8 * q)) {
                r[q] = (r[q] * (255 - a) + cr * a + 127) / 255;
                g[q] = (g[q] * (255 - a) + cg * a + 127) / 255;
                b[q] = (b[q] * (255 - a) + cb * a + 127) / 255;
            }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int y = y0 + 8 * q;
        if (x < W && y < H) {
            uint8_t *o = rast + ((size_t)y * W + x) * 3;
            o[0] = (uint8_t)r[q];
            o[1] = (uint8_t)g[q];
            o[2] = (uint8_t)b[q];
        }
    }
}

}  // namespace

int check_capsules(const ldw_capsule *caps, int64_t n, int W, int H, const char *who) {
    LDW_REQUIRE(W >= 1 && H >= 1 && W <= NET_MAX_DIM && H <= NET_MAX_DIM, LDW_ERR_ARG, "%s: a canvas of %d x %d pixels (1..%d each way)", who, W, H, NET_MAX_DIM);
    LDW_REQUIRE(n >= 0 && n <= NET_MAX_CAPS && (n == 0 || caps), LDW_ERR_ARG, "%s: %lld capsules (0..%lld), or a null list", who, (long long)n, (long long)NET_MAX_CAPS);
    for (int64_t i = 0; i < n; ++i) {
        const ldw_capsule &c = caps[i];
        if (int rc = plot_check_window(c, (long long)i, "capsule", who)) return rc;
        LDW_REQUIRE(c.w >= 1 && c.w <= NET_MAX_W, LDW_ERR_ARG, "%s: capsule %lld has width %d outside 1..%d", who, (long long)i, c.w, NET_MAX_W);
        LDW_REQUIRE(c.alpha >= 1 && c.alpha <= 255 && c.rgb <= 0xFFFFFFu, LDW_ERR_ARG, "%s: capsule %lld has alpha %d outside 1..255 or a colour beyond 0xFFFFFF", who, (long long)i,
                    c.alpha);
    }
    return LDW_OK;
}

// The raster of the capsules, left ON THE DEVICE: *d_rast_out[H][W][3] inside ctx->plot_work, valid until that buffer's next use; the work is queued on the
// context's stream and not waited for.  cv: arrays the caller took for itself beforehand — they are carved from the same buffer, behind which this call
// puts its own, and are bound when it returns.  ev (may be NULL, 3 created events): recorded before the binning, between binning and shading, after it.
int net_raster_device(ldw_ctx *c, Carve &cv, const ldw_capsule *caps, int64_t n, int W, int H, uint8_t **d_rast_out, const Event *ev, const char *who) {
    if (int rc = check_capsules(caps, n, W, H, who)) return rc;
    const int ntx = (W + NET_T - 1) / NET_T, nty = (H + NET_T - 1) / NET_T, ntiles = ntx * nty;
    size_t scan_bytes = 0;
    LDW_HIP(prim_scan_bytes<uint32_t>((size_t)ntiles + 1, c->stream, &scan_bytes));
    auto d_caps = cv.take<ldw_capsule>(n);
    auto d_box = cv.take<TileBox>(n);
    auto d_cnt = cv.take<uint32_t>(ntiles + 1);
    auto d_off = cv.take<uint32_t>(ntiles + 1);
    auto d_tmp = cv.take<uint8_t>((int64_t)scan_bytes);
    auto d_rast = cv.take<uint8_t>((int64_t)W * H * 3);
    if (int rc = cv.reserve(c->plot_work)) return rc;
    if (n > 0) LDW_HIP(hipMemcpyAsync(d_caps, caps, (size_t)n * sizeof(ldw_capsule), hipMemcpyHostToDevice, c->stream));
    if (ev) LDW_HIP(hipEventRecord(ev[0], c->stream));
    LDW_HIP(hipMemsetAsync(d_cnt, 0, (size_t)(ntiles + 1) * 4, c->stream));
    const dim3 bin_grid((ntiles + 255) / 256);
    if (n > 0) {
        LDW_LAUNCH(k_net_boxes, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const ldw_capsule *)d_caps, n, W, H, (TileBox *)d_box);
        LDW_LAUNCH(k_net_bin<0>, bin_grid, dim3(256), 0, c->stream, (const TileBox *)d_box, n, ntx, ntiles, (uint32_t *)d_cnt, (const uint32_t *)nullptr, (uint32_t *)nullptr);
    }
    LDW_HIP(prim_exclusive_sum(d_tmp, scan_bytes, (uint32_t *)d_cnt, (uint32_t *)d_off, (size_t)ntiles + 1, c->stream));
    uint32_t entries = 0;
    LDW_HIP(hipMemcpyAsync(&entries, (uint32_t *)d_off + ntiles, 4, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    // the lists, in a buffer of their own: plot_cols (the carved arrays above stay where they are)
    if (int rc = c->plot_cols.reserve((size_t)std::max<uint32_t>(entries, 1) * 4)) return rc;
    uint32_t *d_list = c->plot_cols.as<uint32_t>();
    if (n > 0) LDW_LAUNCH(k_net_bin<1>, bin_grid, dim3(256), 0, c->stream, (const TileBox *)d_box, n, ntx, ntiles, (uint32_t *)nullptr, (const uint32_t *)d_off, d_list);
    if (ev) LDW_HIP(hipEventRecord(ev[1], c->stream));
    LDW_LAUNCH(k_net_shade, dim3(ntx, nty), dim3(256), 0, c->stream, (const ldw_capsule *)d_caps, (const uint32_t *)d_off, (const uint32_t *)d_list, W, H, (uint8_t *)d_rast);
    if (ev) LDW_HIP(hipEventRecord(ev[2], c->stream));
    *d_rast_out = d_rast;
    return LDW_OK;
}

// the raster of the capsules, rgb_out[H][W][3] (host); ms_out (may be NULL, 2 doubles): hip-event times of the binning and of the shading
int net_raster(ldw_ctx *c, const ldw_capsule *caps, int64_t n, int W, int H, uint8_t *rgb_out, double *ms_out, const char *who) {
    if (int rc = check_capsules(caps, n, W, H, who)) return rc;
    LDW_REQUIRE(rgb_out, LDW_ERR_ARG, "%s: null output", who);
    PlotEvents<3> ev;
    if (ms_out) LDW_HIP(ev.create());
    Carve cv;
    uint8_t *d_rast = nullptr;
    if (int rc = net_raster_device(c, cv, caps, n, W, H, &d_rast, ms_out ? ev.e : nullptr, who)) return rc;
    LDW_HIP(hipMemcpyAsync(rgb_out, d_rast, (size_t)W * H * 3, hipMemcpyDeviceToHost, c->stream));
    LDW_HIP(hipStreamSynchronize(c->stream));
    if (ms_out) LDW_HIP(ev.elapsed(ms_out));
    return LDW_OK;
}

}  // namespace ldw

using namespace ldw;

extern "C" {

int ldw_plot_network(ldw_ctx *c, const ldw_capsule *caps, int64_t n_caps, int32_t W, int32_t H, const int32_t *node_xy, const char *const *node_names, int32_t n_nodes,
                     const char *title, const int32_t *legend_value, const uint32_t *legend_rgb, int32_t n_legend, int32_t text_scale, const char *png_path,
                     uint8_t *rgb_out, int32_t *boxes_out) {
    LDW_REQUIRE(c != nullptr, LDW_ERR_ARG, "ldw_plot_network: null context");
    LDW_REQUIRE(png_path || rgb_out, LDW_ERR_ARG, "ldw_plot_network: neither a path nor a canvas to write to");
    LDW_REQUIRE(n_nodes >= 0 && n_nodes <= (1 << 20) && (n_nodes == 0 || (node_xy && node_names)), LDW_ERR_ARG, "ldw_plot_network: %d nodes, or null node arrays", (int)n_nodes);
    LDW_REQUIRE(n_legend >= 0 && n_legend <= 4096 && (n_legend == 0 || (legend_value && legend_rgb)), LDW_ERR_ARG, "ldw_plot_network: %d legend entries, or null legend arrays",
                (int)n_legend);
    LDW_REQUIRE(text_scale >= 1 && text_scale <= 64, LDW_ERR_ARG, "ldw_plot_network: text scale %d outside 1..64", (int)text_scale);
    for (int k = 0; k < n_nodes; ++k) LDW_REQUIRE(node_names[k] != nullptr, LDW_ERR_ARG, "ldw_plot_network: node %d has no name", k);
    if (int rc = check_capsules(caps, n_caps, W, H, "ldw_plot_network")) return rc;
    if (int rc = check_gpu(c)) return rc;
    PlotCanvas canvas(rgb_out, W, H);
    if (int rc = net_raster(c, caps, n_caps, W, H, canvas.rgb, nullptr, "ldw_plot_network")) return rc;
    plot_net_overlay(canvas.rgb, W, H, node_xy, node_names, n_nodes, title, legend_value, legend_rgb, n_legend, text_scale, boxes_out);
    return canvas.finish(png_path);
}

int ldw_debug_plot_capsules(ldw_ctx *c, const ldw_capsule *caps, int64_t n_caps, int32_t W, int32_t H, uint8_t *rgb_out, double *ms_out) {
    LDW_REQUIRE(c != nullptr, LDW_ERR_ARG, "ldw_debug_plot_capsules: null context");
    if (int rc = check_capsules(caps, n_caps, W, H, "ldw_debug_plot_capsules")) return rc;
    if (int rc = check_gpu(c)) return rc;
    return net_raster(c, caps, n_caps, W, H, rgb_out, ms_out, "ldw_debug_plot_capsules");
}

}  // extern "C"
