// The tanglegram's marks on the device (include/ldweaver_amd.h 12): the links as the network plot's translucent capsules
// (ldw_plot_net.hip, unchanged), then opaque rectangles — the two genome bars and the loci — painted over that raster in list order.
//
// Rule.  A rectangle is the half-open pixel box [x0, x1) x [y0, y1), clipped to the canvas; a pixel takes the colour of the LAST rectangle of the
// list that covers it, a pixel that none covers keeps the capsule raster.  An empty rectangle paints nothing.
//
// Kernels.  "The last rectangle" is a maximum over list indices, and an integer maximum does not depend on the order in which it is taken.  The host
// clips every rectangle and sums the pixel counts (at most 2^16 rectangles: one short loop): pixel t of the whole list belongs to the rectangle b
// with off[b] <= t < off[b + 1] and is pixel t - off[b] of its clipped box, row by row.  k_tng_own walks t = 0 .. off[n] in a grid-stride loop — a
// bar of 10^5 pixels and a locus of a dozen are spread over the threads alike, and the lanes of a wave meet consecutive pixels of a row — and does
// atomicMax(owner[pixel], b + 1) on a zeroed uint32 image.  k_tng_paint walks the same list: the thread whose rectangle owns its pixel writes the
// colour, so every covered pixel is written once and no other pixel of the raster is touched.  A wave looks its first pixel's rectangle up once (a
// binary search over off); a lane whose pixel lies in a later one searches on from there.
//
// Bounds: a pixel of the list lies inside its rectangle's box clipped to [0, W) x [0, H), so inside the owner image and the raster.
#include <algorithm>
#include <vector>

#include "ldw_plot_prim.h"

namespace ldw {
namespace {

constexpr int TNG_BLOCKS = 2048;
constexpr int64_t TNG_MAX_RECTS = 1 << 16;

// the last b in [lo, n) with off[b] <= t, given off[lo] <= t < off[n]
__device__ __forceinline__ int rect_of(const uint64_t *__restrict__ off, int lo, int n, uint64_t t) {
    int hi = n;   // off[hi] > t
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= t)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// pixel t of the list: its rectangle (returned) and its index in the W x H image
__device__ __forceinline__ int rect_pixel(const ldw_rect *__restrict__ rects, const uint64_t *__restrict__ off, int n, int W, int H, uint64_t t, int lane, size_t *pix) {
    int b = rect_of(off, 0, n, t - lane);   // the rectangle of the wave's first pixel: the same loads in every lane
    if (t >= off[b + 1]) b = rect_of(off, b + 1, n, t);
    const ldw_rect r = rects[b];
    const int xa = max(r.x0, 0), ya = max(r.y0, 0), w = min(r.x1, W) - xa;   // w >= 1: an empty box has no pixel in the list
    const uint32_t local = (uint32_t)(t - off[b]);                            // < W H <= 2^26
    *pix = (size_t)(ya + (int)(local / (uint32_t)w)) * W + (xa + (int)(local % (uint32_t)w));
    return b;
}

__global__ __launch_bounds__(256) void k_tng_own(const ldw_rect *__restrict__ rects, const uint64_t *__restrict__ off, int n, int W, int H, uint32_t *__restrict__ owner) {
    const uint64_t total = off[n];
    const int lane = threadIdx.x & 63;
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (uint64_t)gridDim.x * 256) {
        size_t pix;
        const int b = rect_pixel(rects, off, n, W, H, t, lane, &pix);
        atomicMax(&owner[pix], (uint32_t)b + 1);
    }
}

__global__ __launch_bounds__(256) void k_tng_paint(const ldw_rect *__restrict__ rects, const uint64_t *__restrict__ off, int n, int W, int H, const uint32_t *__restrict__ owner,
                                                   uint8_t *__restrict__ rast) {
    const uint64_t total = off[n];
    const int lane = threadIdx.x & 63;
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (uint64_t)gridDim.x * 256) {
        size_t pix;
        const int b = rect_pixel(rects, off, n, W, H, t, lane, &pix);
        if (owner[pix] != (uint32_t)b + 1) continue;
        plot_store_rgb(rast + pix * 3, rects[b].rgb);
    }
}

int check_rects(const ldw_rect *rects, int64_t n, const char *who) {
    LDW_REQUIRE(n >= 0 && n <= TNG_MAX_RECTS && (n == 0 || rects), LDW_ERR_ARG, "%s: %lld rectangles (0..%lld), or a null list", who, (long long)n, (long long)TNG_MAX_RECTS);
    for (int64_t i = 0; i < n; ++i) {
        const ldw_rect &r = rects[i];
        if (int rc = plot_check_window(r, (long long)i, "rectangle", who)) return rc;
        LDW_REQUIRE(r.x1 >= r.x0 && r.y1 >= r.y0, LDW_ERR_ARG, "%s: rectangle %lld has x1 < x0 or y1 < y0", who, (long long)i);
        LDW_REQUIRE(r.rgb <= 0xFFFFFFu, LDW_ERR_ARG, "%s: rectangle %lld has a colour beyond 0xFFFFFF", who, (long long)i);
    }
    return LDW_OK;
}

// the capsules, then the rectangles over them: rgb_out[H][W][3] (host).  ms_out (may be NULL, 3 doubles): binning, shading, rectangles
int tng_raster(ldw_ctx *c, const ldw_capsule *caps, int64_t n_caps, const ldw_rect *rects, int64_t n_rects, int W, int H, uint8_t *rgb_out, double *ms_out,
               const char *who) {
    LDW_REQUIRE(rgb_out, LDW_ERR_ARG, "%s: null output", who);
    const int n = (int)n_rects;
    std::vector<uint64_t> off((size_t)n + 1, 0);   // off[b] = pixels of the clipped rectangles before b
    for (int b = 0; b < n; ++b) {
        const ldw_rect &r = rects[b];
        const int64_t w = std::min<int64_t>(r.x1, W) - std::max<int64_t>(r.x0, 0), h = std::min<int64_t>(r.y1, H) - std::max<int64_t>(r.y0, 0);
        off[(size_t)b + 1] = off[(size_t)b] + (w > 0 && h > 0 ? (uint64_t)(w * h) : 0);
    }
    const uint64_t total = off[(size_t)n];
    PlotEvents<4> ev;
    if (ms_out) LDW_HIP(ev.create());
    Carve cv;
    auto d_rects = cv.take<ldw_rect>(n);
    auto d_off = cv.take<uint64_t>(n + 1);
    auto d_owner = cv.take<uint32_t>(total ? (int64_t)W * H : 0);
    uint8_t *d_rast = nullptr;
    if (int rc = net_raster_device(c, cv, caps, n_caps, W, H, &d_rast, ms_out ? ev.e : nullptr, who)) return rc;
    hipStream_t st = c->stream;
    if (total) {
        LDW_HIP(hipMemcpyAsync(d_rects, rects, (size_t)n * sizeof(ldw_rect), hipMemcpyHostToDevice, st));
        LDW_HIP(hipMemcpyAsync(d_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, st));
        LDW_HIP(hipMemsetAsync(d_owner, 0, (size_t)W * H * 4, st));
        const dim3 grid((unsigned)std::min<uint64_t>((total + 255) / 256, TNG_BLOCKS));
        LDW_LAUNCH(k_tng_own, grid, dim3(256), 0, st, (const ldw_rect *)d_rects, (const uint64_t *)d_off, n, W, H, (uint32_t *)d_owner);
        LDW_LAUNCH(k_tng_paint, grid, dim3(256), 0, st, (const ldw_rect *)d_rects, (const uint64_t *)d_off, n, W, H, (const uint32_t *)d_owner, d_rast);
    }
    if (ms_out) LDW_HIP(hipEventRecord(ev.e[3], st));
    LDW_HIP(hipMemcpyAsync(rgb_out, d_rast, (size_t)W * H * 3, hipMemcpyDeviceToHost, st));
    LDW_HIP(hipStreamSynchronize(st));   // (off and the caller's lists were read by the copies above)
    if (ms_out) LDW_HIP(ev.elapsed(ms_out));
    return LDW_OK;
}

}  // namespace
}  // namespace ldw

using namespace ldw;

extern "C" {

int ldw_plot_tanglegram(ldw_ctx *c, const ldw_capsule *caps, int64_t n_caps, const ldw_rect *rects, int64_t n_rects, int32_t W, int32_t H, const int32_t *label_xy,
                        const char *const *labels, int32_t n_labels, const char *title, int32_t text_scale, const char *png_path, uint8_t *rgb_out, int32_t *boxes_out) {
    LDW_REQUIRE(c != nullptr, LDW_ERR_ARG, "ldw_plot_tanglegram: null context");
    LDW_REQUIRE(png_path || rgb_out, LDW_ERR_ARG, "ldw_plot_tanglegram: neither a path nor a canvas to write to");
    LDW_REQUIRE(n_labels >= 0 && n_labels <= (1 << 20) && (n_labels == 0 || (label_xy && labels)), LDW_ERR_ARG, "ldw_plot_tanglegram: %d labels, or null label arrays",
                (int)n_labels);
    LDW_REQUIRE(text_scale >= 1 && text_scale <= 64, LDW_ERR_ARG, "ldw_plot_tanglegram: text scale %d outside 1..64", (int)text_scale);
    for (int k = 0; k < n_labels; ++k) LDW_REQUIRE(labels[k] != nullptr, LDW_ERR_ARG, "ldw_plot_tanglegram: label %d is null", k);
    if (int rc = check_capsules(caps, n_caps, W, H, "ldw_plot_tanglegram")) return rc;
    if (int rc = check_rects(rects, n_rects, "ldw_plot_tanglegram")) return rc;
    if (int rc = check_gpu(c)) return rc;
    PlotCanvas canvas(rgb_out, W, H);
    if (int rc = tng_raster(c, caps, n_caps, rects, n_rects, W, H, canvas.rgb, nullptr, "ldw_plot_tanglegram")) return rc;
    plot_tng_overlay(canvas.rgb, W, H, label_xy, labels, n_labels, title, text_scale, boxes_out);
    return canvas.finish(png_path);
}

int ldw_debug_plot_marks(ldw_ctx *c, const ldw_capsule *caps, int64_t n_caps, const ldw_rect *rects, int64_t n_rects, int32_t W, int32_t H, uint8_t *rgb_out, double *ms_out) {
    LDW_REQUIRE(c != nullptr, LDW_ERR_ARG, "ldw_debug_plot_marks: null context");
    if (int rc = check_capsules(caps, n_caps, W, H, "ldw_debug_plot_marks")) return rc;
    if (int rc = check_rects(rects, n_rects, "ldw_debug_plot_marks")) return rc;
    if (int rc = check_gpu(c)) return rc;
    return tng_raster(c, caps, n_caps, rects, n_rects, W, H, rgb_out, ms_out, "ldw_debug_plot_marks");
}

}  // extern "C"
