// The plots (include/ldweaver_amd.h 12): what the device render (ldw_plot.hip) and the host frame / PNG writer (ldw_png.cpp) share.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/ldweaver_amd.h"
#include "ldw_carve.h"
#include "ldw_own.h"

namespace ldw {

constexpr uint32_t PLOT_BG = 0xFFFFFF, PLOT_GRID = 0xEBEBEB, PLOT_BORDER = 0xB3B3B3, PLOT_TEXT = 0x4D4D4D, PLOT_TITLE = 0x000000,
                   PLOT_GREY = 0xC0C0C0;
constexpr int PLOT_RAMP_N = 2056;

// rev(brewer.pal(6, "RdYlBu")), piecewise linear in sRGB: s = min(floor(5 t), 4), f = 5 t - s, channel = floor(c[s] + (c[s+1] - c[s]) f + 0.5).
// One IEEE operation at a time (the tests compare with numpy), on the host and on the device.
__host__ __device__ __forceinline__ uint32_t plot_gradient(double t) {
#pragma clang fp contract(off)
    constexpr int c[6][3] = {{0x45, 0x75, 0xB4}, {0x91, 0xBF, 0xDB}, {0xE0, 0xF3, 0xF8}, {0xFE, 0xE0, 0x90}, {0xFC, 0x8D, 0x59}, {0xD7, 0x30, 0x27}};
    const double t5 = 5.0 * t;
    int s = (int)floor(t5);
    s = s > 4 ? 4 : (s < 0 ? 0 : s);
    const double f = t5 - (double)s;
    uint32_t rgb = 0;
    for (int k = 0; k < 3; ++k) {
        const double d = (double)(c[s + 1][k] - c[s][k]);
        const double m = d * f;
        const double v = ((double)c[s][k] + m) + 0.5;
        rgb = (rgb << 8) | (uint32_t)(int)floor(v);
    }
    return rgb;
}

// the pixel rule of one axis: min(n - 1, (int)floor((v - v0) / (v1 - v0) * n))
__host__ __device__ __forceinline__ int plot_pixel(double v, double v0, double v1, int n) {
#pragma clang fp contract(off)
    const double a = v - v0;
    const double q = a / (v1 - v0);
    const double p = floor(q * (double)n);
    if (!(p >= 0.0)) return 0;   // (not reached by a kept row: its value lies inside the axis range)
    return p >= (double)n ? n - 1 : (int)p;
}

// host side (ldw_png.cpp)
void plot_ramp_table(uint8_t *rgb);   // PLOT_RAMP_N x 3
int plot_axis(double lo, double hi, int npx, int flip, double lim[2], double *tick, int32_t *px, int32_t *n);
// the frame round the panels, drawn into canvas[height][width][3]; rasters: [n_panels][panel_h][panel_w][3]
void plot_frame(uint8_t *canvas, const ldw_plot_layout &lay, int kind, const uint8_t *rasters, const int32_t *panel_label, const char *title,
                bool cbar_valid, double cb_lo, double cb_hi);

// the frame of an xy figure (ldw_plot_xy.hip) round its one panel: ticks, title, axis labels and, for LDW_PLOT_CDS, the legend "Cluster"
void plot_xy_frame(uint8_t *canvas, const ldw_plot_layout &lay, int kind, const uint8_t *raster, const char *title, const char *xlab, const char *ylab,
                   const uint32_t *class_rgb, int n_classes);

// the network plot's node labels, title and legend over the edge raster canvas[H][W][3]; boxes (may be NULL): (n_nodes + 2) x 4
void plot_net_overlay(uint8_t *canvas, int W, int H, const int32_t *node_xy, const char *const *node_names, int n_nodes, const char *title,
                      const int32_t *legend_value, const uint32_t *legend_rgb, int n_legend, int scale, int32_t *boxes);

// N hip events of a timed render: created on demand, destroyed with the object
template <int N> struct PlotEvents {
    Event e[N];
    hipError_t create() {
        for (Event &x : e)
            if (hipError_t rc = x.ensure()) return rc;
        return hipSuccess;
    }
    // ms[k] = the time from event k to event k + 1 (all recorded, the stream idle)
    hipError_t elapsed(double *ms) const {
        for (int k = 0; k + 1 < N; ++k) {
            float f = 0;
            if (hipError_t rc = hipEventElapsedTime(&f, e[k], e[k + 1])) return rc;
            ms[k] = f;
        }
        return hipSuccess;
    }
};

// ldw_plot_net.hip, shared with the tanglegram (ldw_plot_tng.hip): the capsule checks, and the capsule raster left on the device (see there)
int check_capsules(const ldw_capsule *caps, int64_t n, int W, int H, const char *who);
int net_raster_device(ldw_ctx *c, Carve &cv, const ldw_capsule *caps, int64_t n, int W, int H, uint8_t **d_rast_out, const Event *ev, const char *who);

// the tanglegram's labels (read upwards from their anchors label_xy[2 k], label_xy[2 k + 1]) and title over the device canvas[H][W][3]
// (ldw_plot_tng.hip); boxes (may be NULL): (n_labels + 1) x 4
void plot_tng_overlay(uint8_t *canvas, int W, int H, const int32_t *label_xy, const char *const *labels, int n_labels, const char *title, int scale,
                      int32_t *boxes);

// the tree view's band labels, title and two legends over the device canvas[H][W][3] (ldw_plot_tree.hip); boxes (may be NULL): (n_bands + 3) x 4
void plot_tree_overlay(uint8_t *canvas, int W, int H, const int32_t *band_rect, const char *const *band_label, int n_bands, const char *title,
                       const char *const *legend_title, const int32_t *legend_n, const char *const *legend_label, const uint32_t *legend_rgb,
                       const int32_t *legend_xy, int scale, int32_t *boxes);

}  // namespace ldw
