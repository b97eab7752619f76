// Host side of the plots (include/ldweaver_amd.h 12): the figure layout, the frame round the device-rendered panels (a stand-in for ggplot's
// theme_light, not a copy of it), a 5 x 7 bitmap font and the PNG writer over zlib.  Nothing here needs a context or a GPU.
#include <stdio.h>
#include <string.h>
#include <zlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ldw_internal.h"
#include "ldw_plot.h"

#pragma clang fp contract(off)

namespace ldw {

// ---- colours ------------------------------------------------------------------------------------------------------------------------------

// colorRampPalette(c("white", "#E1B9B4", "#AE452C", "#802418"))(2056): linear in RGB between the four stops, rounded half up
void plot_ramp_table(uint8_t *rgb) {
    static const int c[4][3] = {{0xFF, 0xFF, 0xFF}, {0xE1, 0xB9, 0xB4}, {0xAE, 0x45, 0x2C}, {0x80, 0x24, 0x18}};
    for (int i = 0; i < PLOT_RAMP_N; ++i) {
        const double t = (double)i / (double)(PLOT_RAMP_N - 1);
        const double p = 3.0 * t;
        int s = (int)floor(p);
        s = s > 2 ? 2 : s;
        const double f = p - (double)s;
        for (int k = 0; k < 3; ++k) {
            const double m = (double)(c[s + 1][k] - c[s][k]) * f;
            const double v = ((double)c[s][k] + m) + 0.5;
            rgb[i * 3 + k] = (uint8_t)(int)floor(v);
        }
    }
}

// ---- axes ---------------------------------------------------------------------------------------------------------------------------------

// axis range = data range widened by 5 % on both sides (zero width: +-0.5 first); ticks at the multiples of a 1-2-5 step of about a fifth
// of the range that lie inside it
int plot_axis(double lo, double hi, int npx, int flip, double lim[2], double *tick, int32_t *px, int32_t *n_out) {
    if (!(std::isfinite(lo) && std::isfinite(hi) && lo <= hi) || npx < 1) return LDW_ERR_ARG;
    if (hi == lo) {
        lo = lo - 0.5;
        hi = hi + 0.5;
    }
    const double d = (hi - lo) * 0.05;
    const double x0 = lo - d, x1 = hi + d;
    if (!(std::isfinite(x0) && std::isfinite(x1) && std::isfinite(x1 - x0) && x1 > x0)) return LDW_ERR_ARG;   // (ranges near DBL_MAX)
    lim[0] = x0;
    lim[1] = x1;
    int n = 0;
    const double raw = (x1 - x0) / 5.0;
    if (std::isfinite(raw) && raw > 0 && raw > 1e-300) {
        int e = (int)floor(log10(raw));
        double m = raw / pow(10.0, e);
        int mult = m < 1.5 ? 1 : (m < 3.5 ? 2 : (m < 7.5 ? 5 : 10));
        if (mult == 10) {
            mult = 1;
            e += 1;
        }
        const double p10 = pow(10.0, e < 0 ? -e : e);
        auto value = [&](double k) { return e < 0 ? (k * mult) / p10 : (k * mult) * p10; };
        const double step = value(1.0);
        double k0 = ceil(x0 / step), k1 = floor(x1 / step);
        while (value(k0) < x0) k0 += 1;
        while (value(k1) > x1) k1 -= 1;
        for (double k = k0; k <= k1 && n < LDW_PLOT_MAX_TICKS; k += 1) {
            const double v = value(k);
            tick[n] = v == 0 ? 0.0 : v;
            const int i = plot_pixel(v, x0, x1, npx);
            px[n] = flip ? npx - 1 - i : i;
            ++n;
        }
    }
    *n_out = n;
    return LDW_OK;
}

// ---- drawing on the host canvas -------------------------------------------------------------------------------------------------------------

namespace {

struct Canvas {
    uint8_t *p;
    int w, h;
    void px(int x, int y, uint32_t rgb) {
        if (x < 0 || y < 0 || x >= w || y >= h) return;
        uint8_t *q = p + ((size_t)y * w + x) * 3;
        q[0] = (uint8_t)(rgb >> 16);
        q[1] = (uint8_t)(rgb >> 8);
        q[2] = (uint8_t)rgb;
    }
    void rect(int x, int y, int rw, int rh, uint32_t rgb) {
        for (int j = y; j < y + rh; ++j)
            for (int i = x; i < x + rw; ++i) px(i, j, rgb);
    }
};

// 5 x 7 glyphs of the printable ASCII characters 0x20..0x7E, one byte per column, bit 0 = top row
const uint8_t FONT[95][5] = {
    {0x00, 0x00, 0x00, 0x00, 0x00}, {0x00, 0x00, 0x5F, 0x00, 0x00}, {0x00, 0x07, 0x00, 0x07, 0x00}, {0x14, 0x7F, 0x14, 0x7F, 0x14},
    {0x24, 0x2A, 0x7F, 0x2A, 0x12}, {0x23, 0x13, 0x08, 0x64, 0x62}, {0x36, 0x49, 0x56, 0x20, 0x50}, {0x00, 0x08, 0x07, 0x03, 0x00},
    {0x00, 0x1C, 0x22, 0x41, 0x00}, {0x00, 0x41, 0x22, 0x1C, 0x00}, {0x2A, 0x1C, 0x7F, 0x1C, 0x2A}, {0x08, 0x08, 0x3E, 0x08, 0x08},
    {0x00, 0x50, 0x30, 0x00, 0x00}, {0x08, 0x08, 0x08, 0x08, 0x08}, {0x00, 0x00, 0x60, 0x60, 0x00}, {0x20, 0x10, 0x08, 0x04, 0x02},
    {0x3E, 0x51, 0x49, 0x45, 0x3E}, {0x00, 0x42, 0x7F, 0x40, 0x00}, {0x72, 0x49, 0x49, 0x49, 0x46}, {0x21, 0x41, 0x49, 0x4D, 0x33},
    {0x18, 0x14, 0x12, 0x7F, 0x10}, {0x27, 0x45, 0x45, 0x45, 0x39}, {0x3C, 0x4A, 0x49, 0x49, 0x31}, {0x41, 0x21, 0x11, 0x09, 0x07},
    {0x36, 0x49, 0x49, 0x49, 0x36}, {0x46, 0x49, 0x49, 0x29, 0x1E}, {0x00, 0x00, 0x14, 0x00, 0x00}, {0x00, 0x40, 0x34, 0x00, 0x00},
    {0x00, 0x08, 0x14, 0x22, 0x41}, {0x14, 0x14, 0x14, 0x14, 0x14}, {0x00, 0x41, 0x22, 0x14, 0x08}, {0x02, 0x01, 0x59, 0x09, 0x06},
    {0x3E, 0x41, 0x5D, 0x59, 0x4E}, {0x7C, 0x12, 0x11, 0x12, 0x7C}, {0x7F, 0x49, 0x49, 0x49, 0x36}, {0x3E, 0x41, 0x41, 0x41, 0x22},
    {0x7F, 0x41, 0x41, 0x41, 0x3E}, {0x7F, 0x49, 0x49, 0x49, 0x41}, {0x7F, 0x09, 0x09, 0x09, 0x01}, {0x3E, 0x41, 0x41, 0x51, 0x73},
    {0x7F, 0x08, 0x08, 0x08, 0x7F}, {0x00, 0x41, 0x7F, 0x41, 0x00}, {0x20, 0x40, 0x41, 0x3F, 0x01}, {0x7F, 0x08, 0x14, 0x22, 0x41},
    {0x7F, 0x40, 0x40, 0x40, 0x40}, {0x7F, 0x02, 0x1C, 0x02, 0x7F}, {0x7F, 0x04, 0x08, 0x10, 0x7F}, {0x3E, 0x41, 0x41, 0x41, 0x3E},
    {0x7F, 0x09, 0x09, 0x09, 0x06}, {0x3E, 0x41, 0x51, 0x21, 0x5E}, {0x7F, 0x09, 0x19, 0x29, 0x46}, {0x26, 0x49, 0x49, 0x49, 0x32},
    {0x03, 0x01, 0x7F, 0x01, 0x03}, {0x3F, 0x40, 0x40, 0x40, 0x3F}, {0x1F, 0x20, 0x40, 0x20, 0x1F}, {0x3F, 0x40, 0x38, 0x40, 0x3F},
    {0x63, 0x14, 0x08, 0x14, 0x63}, {0x03, 0x04, 0x78, 0x04, 0x03}, {0x61, 0x59, 0x49, 0x4D, 0x43}, {0x00, 0x7F, 0x41, 0x41, 0x41},
    {0x02, 0x04, 0x08, 0x10, 0x20}, {0x00, 0x41, 0x41, 0x41, 0x7F}, {0x04, 0x02, 0x01, 0x02, 0x04}, {0x40, 0x40, 0x40, 0x40, 0x40},
    {0x00, 0x03, 0x07, 0x08, 0x00}, {0x20, 0x54, 0x54, 0x78, 0x40}, {0x7F, 0x28, 0x44, 0x44, 0x38}, {0x38, 0x44, 0x44, 0x44, 0x28},
    {0x38, 0x44, 0x44, 0x28, 0x7F}, {0x38, 0x54, 0x54, 0x54, 0x18}, {0x00, 0x08, 0x7E, 0x09, 0x02}, {0x0C, 0x52, 0x52, 0x52, 0x3E},
    {0x7F, 0x08, 0x04, 0x04, 0x78}, {0x00, 0x44, 0x7D, 0x40, 0x00}, {0x20, 0x40, 0x40, 0x3D, 0x00}, {0x7F, 0x10, 0x28, 0x44, 0x00},
    {0x00, 0x41, 0x7F, 0x40, 0x00}, {0x7C, 0x04, 0x78, 0x04, 0x78}, {0x7C, 0x08, 0x04, 0x04, 0x78}, {0x38, 0x44, 0x44, 0x44, 0x38},
    {0x7C, 0x14, 0x14, 0x14, 0x08}, {0x08, 0x14, 0x14, 0x18, 0x7C}, {0x7C, 0x08, 0x04, 0x04, 0x08}, {0x48, 0x54, 0x54, 0x54, 0x24},
    {0x04, 0x04, 0x3F, 0x44, 0x24}, {0x3C, 0x40, 0x40, 0x20, 0x7C}, {0x1C, 0x20, 0x40, 0x20, 0x1C}, {0x3C, 0x40, 0x30, 0x40, 0x3C},
    {0x44, 0x28, 0x10, 0x28, 0x44}, {0x0C, 0x50, 0x50, 0x50, 0x3C}, {0x44, 0x64, 0x54, 0x4C, 0x44}, {0x00, 0x08, 0x36, 0x41, 0x00},
    {0x00, 0x00, 0x77, 0x00, 0x00}, {0x00, 0x41, 0x36, 0x08, 0x00}, {0x02, 0x01, 0x02, 0x04, 0x02},
};

int text_width(const char *s, int scale) {
    const int n = (int)strlen(s);
    return n ? n * 6 * scale - scale : 0;
}

// text with its top-left corner at (x, y); up != 0: rotated a quarter turn counter-clockwise, reading upwards from (x, y) = its bottom-left
void draw_text(Canvas &cv, int x, int y, const char *s, int scale, uint32_t rgb, int up = 0) {
    for (int k = 0; s[k]; ++k) {
        const unsigned ch = (unsigned char)s[k];
        const uint8_t *g = FONT[ch >= 0x20 && ch <= 0x7E ? ch - 0x20 : '?' - 0x20];
        for (int col = 0; col < 5; ++col)
            for (int row = 0; row < 7; ++row) {
                if (!((g[col] >> row) & 1)) continue;
                const int u = (k * 6 + col) * scale, v = row * scale;   // along the text, across it
                if (up)
                    cv.rect(x + v, y - u - scale + 1, scale, scale, rgb);
                else
                    cv.rect(x + u, y + v, scale, scale, rgb);
            }
    }
}

std::string fmt_tick(double v) {
    char buf[48];
    snprintf(buf, sizeof(buf), "%g", v);
    return buf;
}

}  // namespace

void plot_frame(uint8_t *canvas, const ldw_plot_layout &lay, int kind, const uint8_t *rasters, const int32_t *panel_label, const char *title,
                bool cbar_valid, double cb_lo, double cb_hi) {
    Canvas cv{canvas, lay.width, lay.height};
    memset(canvas, 0xFF, (size_t)lay.width * lay.height * 3);
    const int pw = lay.panel_w, ph = lay.panel_h;
    const int sc = kind == LDW_PLOT_LDMAP ? 10 : 3, tick_len = 8;
    for (int p = 0; p < lay.n_panels; ++p) {
        const int x = lay.panel[p][0], y = lay.panel[p][1];
        cv.rect(x - 1, y - 1, pw + 2, ph + 2, PLOT_BORDER);
        for (int j = 0; j < ph; ++j) memcpy(canvas + ((size_t)(y + j) * lay.width + x) * 3, rasters + ((size_t)p * ph + j) * pw * 3, (size_t)pw * 3);
        if (lay.strip[p][2] > 0) {
            cv.rect(lay.strip[p][0], lay.strip[p][1], lay.strip[p][2], lay.strip[p][3], PLOT_BORDER);
            char buf[24];
            snprintf(buf, sizeof(buf), "%d", panel_label ? (int)panel_label[p] : p + 1);
            draw_text(cv, lay.strip[p][0] + (lay.strip[p][2] - text_width(buf, sc)) / 2, lay.strip[p][1] + (lay.strip[p][3] - 7 * sc) / 2, buf, sc, PLOT_BG);
        }
        const int col = p % lay.cols;
        const bool below = p + lay.cols < lay.n_panels;   // a panel lies under this one
        for (int t = 0; t < lay.n_yticks; ++t) {
            if (col != 0) break;
            const int ty = y + lay.ytick_px[t];
            cv.rect(x - 1 - tick_len, ty, tick_len, 1, PLOT_BORDER);
            const std::string s = fmt_tick(lay.ytick[t]);
            draw_text(cv, x - 1 - tick_len - 6 - text_width(s.c_str(), sc), ty - (7 * sc) / 2, s.c_str(), sc, PLOT_TEXT);
        }
        for (int t = 0; t < lay.n_xticks; ++t) {
            if (below) break;
            const int tx = x + lay.xtick_px[t];
            cv.rect(tx, y + ph + 1, 1, tick_len, PLOT_BORDER);
            const std::string s = fmt_tick(lay.xtick[t]);
            draw_text(cv, tx - text_width(s.c_str(), sc) / 2, y + ph + 1 + tick_len + 6, s.c_str(), sc, PLOT_TEXT);
        }
    }
    if (kind != LDW_PLOT_LDMAP) {
        // axis titles: centred under / beside the block of panels
        int x_lo = lay.width, x_hi = 0, y_lo = lay.height, y_hi = 0;
        for (int p = 0; p < lay.n_panels; ++p) {
            x_lo = std::min(x_lo, lay.panel[p][0]);
            x_hi = std::max(x_hi, lay.panel[p][0] + pw);
            y_lo = std::min(y_lo, lay.panel[p][1]);
            y_hi = std::max(y_hi, lay.panel[p][1] + ph);
        }
        const char *xt = "Basepair separation", *yt = "MI";
        const int st = 4;
        draw_text(cv, (x_lo + x_hi - text_width(xt, st)) / 2, lay.height - 12 - 7 * st, xt, st, PLOT_TITLE);
        draw_text(cv, 12, (y_lo + y_hi + text_width(yt, st)) / 2, yt, st, PLOT_TITLE, 1);
    } else if (title && title[0]) {
        draw_text(cv, (lay.width - text_width(title, sc)) / 2, (lay.panel[0][1] - 7 * sc) / 2, title, sc, PLOT_TITLE);
    }
    if (lay.cbar[2] > 0) {
        const int x = lay.cbar[0], y = lay.cbar[1], w = lay.cbar[2], h = lay.cbar[3];
        for (int j = 0; j < h; ++j) {
            const double t = h > 1 ? (double)(h - 1 - j) / (double)(h - 1) : 0.5;
            cv.rect(x, y + j, w, 1, plot_gradient(t));
        }
        draw_text(cv, x, y - 14 - 7 * sc, "srp_max", sc, PLOT_TITLE);
        if (cbar_valid) {
            draw_text(cv, x + w + 8, y, fmt_tick(cb_hi).c_str(), sc, PLOT_TEXT);
            draw_text(cv, x + w + 8, y + h - 7 * sc, fmt_tick(cb_lo).c_str(), sc, PLOT_TEXT);
        }
    }
}

// The frame of an xy figure (ldw_plot_xy.hip): the panel's border, ticks and tick labels as in plot_frame; xlab centred under the panel and ylab
// read upwards beside it; the title (LDW_PLOT_FIT) centred above the panel; for LDW_PLOT_CDS the legend "Cluster" right of the panel, one square
// swatch and the class number (from 1) per class.  NULL or empty strings draw nothing.
void plot_xy_frame(uint8_t *canvas, const ldw_plot_layout &lay, int kind, const uint8_t *raster, const char *title, const char *xlab, const char *ylab,
                   const uint32_t *class_rgb, int n_classes) {
    Canvas cv{canvas, lay.width, lay.height};
    memset(canvas, 0xFF, (size_t)lay.width * lay.height * 3);
    const int pw = lay.panel_w, ph = lay.panel_h, x = lay.panel[0][0], y = lay.panel[0][1];
    const int sc = 3, st = 4, tick_len = 8;
    cv.rect(x - 1, y - 1, pw + 2, ph + 2, PLOT_BORDER);
    for (int j = 0; j < ph; ++j) memcpy(canvas + ((size_t)(y + j) * lay.width + x) * 3, raster + (size_t)j * pw * 3, (size_t)pw * 3);
    for (int t = 0; t < lay.n_yticks; ++t) {
        const int ty = y + lay.ytick_px[t];
        cv.rect(x - 1 - tick_len, ty, tick_len, 1, PLOT_BORDER);
        const std::string s = fmt_tick(lay.ytick[t]);
        draw_text(cv, x - 1 - tick_len - 6 - text_width(s.c_str(), sc), ty - (7 * sc) / 2, s.c_str(), sc, PLOT_TEXT);
    }
    for (int t = 0; t < lay.n_xticks; ++t) {
        const int tx = x + lay.xtick_px[t];
        cv.rect(tx, y + ph + 1, 1, tick_len, PLOT_BORDER);
        const std::string s = fmt_tick(lay.xtick[t]);
        draw_text(cv, tx - text_width(s.c_str(), sc) / 2, y + ph + 1 + tick_len + 6, s.c_str(), sc, PLOT_TEXT);
    }
    if (xlab && xlab[0]) draw_text(cv, x + (pw - text_width(xlab, st)) / 2, lay.height - 12 - 7 * st, xlab, st, PLOT_TITLE);
    if (ylab && ylab[0]) draw_text(cv, 12, y + (ph + text_width(ylab, st)) / 2, ylab, st, PLOT_TITLE, 1);
    if (kind == LDW_PLOT_FIT && title && title[0]) draw_text(cv, x + (pw - text_width(title, st)) / 2, (y - 7 * st) / 2, title, st, PLOT_TITLE);
    if (kind == LDW_PLOT_CDS) {
        const int th = 7 * sc, gap = 2 * sc, lx = x + pw + 50;
        const int ly = y + (ph - (n_classes + 1) * (th + gap)) / 2;
        draw_text(cv, lx, ly, "Cluster", sc, PLOT_TITLE);
        for (int k = 0; k < n_classes; ++k) {
            const int yk = ly + (k + 1) * (th + gap);
            cv.rect(lx, yk, th, th, class_rgb[k]);
            draw_text(cv, lx + th + gap, yk, std::to_string(k + 1).c_str(), sc, PLOT_TEXT);
        }
    }
}

// The network plot's text over the edge raster (ldw_plot_net.hip): a white, bordered box with the node's name centred on every node, the title
// centred at the top, and at the bottom the legend "Num_Links" with one swatch and value per colour.  boxes (may be NULL): x, y, w, h of the node
// boxes in node order, then of the title and of the legend (w = 0: not drawn).
void plot_net_overlay(uint8_t *canvas, int W, int H, const int32_t *node_xy, const char *const *node_names, int n_nodes, const char *title,
                      const int32_t *legend_value, const uint32_t *legend_rgb, int n_legend, int sc, int32_t *boxes) {
    Canvas cv{canvas, W, H};
    const int pad = 2 * sc, th = 7 * sc, line = std::max(1, sc / 2);
    auto note = [&](int k, int x, int y, int w, int h) {
        if (!boxes) return;
        boxes[4 * k] = x;
        boxes[4 * k + 1] = y;
        boxes[4 * k + 2] = w;
        boxes[4 * k + 3] = h;
    };
    for (int k = 0; k < n_nodes; ++k) {
        const int tw = text_width(node_names[k], sc), bw = tw + 2 * pad, bh = th + 2 * pad;
        const int x = node_xy[2 * k] - bw / 2, y = node_xy[2 * k + 1] - bh / 2;
        cv.rect(x, y, bw, bh, PLOT_TEXT);
        cv.rect(x + line, y + line, bw - 2 * line, bh - 2 * line, PLOT_BG);
        draw_text(cv, x + pad, y + pad, node_names[k], sc, PLOT_TITLE);
        note(k, x, y, bw, bh);
    }
    if (title && title[0]) {
        const int st = sc + sc / 2, tw = text_width(title, st);
        const int x = (W - tw) / 2, y = 2 * sc;
        cv.rect(x - pad, y - pad, tw + 2 * pad, 7 * st + 2 * pad, PLOT_BG);
        draw_text(cv, x, y, title, st, PLOT_TITLE);
        note(n_nodes, x - pad, y - pad, tw + 2 * pad, 7 * st + 2 * pad);
    } else {
        note(n_nodes, 0, 0, 0, 0);
    }
    if (n_legend > 0) {
        const char *name = "Num_Links";
        const int sw = 4 * th, gap = 2 * sc;
        std::vector<std::string> val((size_t)n_legend);
        int total = text_width(name, sc);
        for (int k = 0; k < n_legend; ++k) {
            val[(size_t)k] = std::to_string(legend_value[k]);
            total += 2 * gap + sw + gap + text_width(val[(size_t)k].c_str(), sc);
        }
        int x = (W - total) / 2;
        const int y = H - 2 * sc - th - pad;
        cv.rect(x - pad, y - pad, total + 2 * pad, th + 2 * pad, PLOT_BG);
        note(n_nodes + 1, x - pad, y - pad, total + 2 * pad, th + 2 * pad);
        draw_text(cv, x, y, name, sc, PLOT_TITLE);
        x += text_width(name, sc);
        for (int k = 0; k < n_legend; ++k) {
            x += 2 * gap;
            cv.rect(x, y + th / 2 - sc, sw, 2 * sc, legend_rgb[k]);
            x += sw + gap;
            draw_text(cv, x, y, val[(size_t)k].c_str(), sc, PLOT_TEXT);
            x += text_width(val[(size_t)k].c_str(), sc);
        }
    } else {
        note(n_nodes + 1, 0, 0, 0, 0);
    }
}

// The tree view's text over the device canvas (ldw_plot_tree.hip): left of every band its label, right-aligned 2 scale pixels before the band and
// centred on its height; the title centred at the top; two legends, each its title over one square swatch and label per entry, with the top-left
// corner at legend_xy[2 k], legend_xy[2 k + 1] (entries of legend 1 follow those of legend 0 in legend_label / legend_rgb).  boxes (may be NULL):
// x, y, w, h of the band labels in band order, then of the title and of the two legends (w = 0: not drawn); a box may reach past the canvas.
void plot_tree_overlay(uint8_t *canvas, int W, int H, const int32_t *band_rect, const char *const *band_label, int n_bands, const char *title,
                       const char *const *legend_title, const int32_t *legend_n, const char *const *legend_label, const uint32_t *legend_rgb,
                       const int32_t *legend_xy, int sc, int32_t *boxes) {
    Canvas cv{canvas, W, H};
    const int th = 7 * sc, gap = 2 * sc;
    auto note = [&](int k, int x, int y, int w, int h) {
        if (!boxes) return;
        boxes[4 * k] = x;
        boxes[4 * k + 1] = y;
        boxes[4 * k + 2] = w;
        boxes[4 * k + 3] = h;
    };
    for (int r = 0; r < n_bands; ++r) {
        const char *s = band_label ? band_label[r] : nullptr;
        if (!s || !s[0]) {
            note(r, 0, 0, 0, 0);
            continue;
        }
        const int tw = text_width(s, sc);
        const int x = band_rect[4 * r] - gap - tw, y = band_rect[4 * r + 1] + (band_rect[4 * r + 3] - th) / 2;
        draw_text(cv, x, y, s, sc, PLOT_TEXT);
        note(r, x, y, tw, th);
    }
    if (title && title[0]) {
        const int st = sc + sc / 2, tw = text_width(title, st);
        const int x = (W - tw) / 2, y = 2 * sc;
        draw_text(cv, x, y, title, st, PLOT_TITLE);
        note(n_bands, x, y, tw, 7 * st);
    } else {
        note(n_bands, 0, 0, 0, 0);
    }
    int first = 0;
    for (int k = 0; k < 2; ++k) {
        const int n = legend_n[k];
        if (n <= 0) {
            note(n_bands + 1 + k, 0, 0, 0, 0);
            continue;
        }
        const char *name = legend_title[k] ? legend_title[k] : "";
        const int x = legend_xy[2 * k], y = legend_xy[2 * k + 1];
        int w = text_width(name, sc);
        draw_text(cv, x, y, name, sc, PLOT_TITLE);
        for (int j = 0; j < n; ++j) {
            const int yj = y + (j + 1) * (th + gap);
            cv.rect(x, yj, th, th, legend_rgb[first + j]);
            draw_text(cv, x + th + gap, yj, legend_label[first + j], sc, PLOT_TEXT);
            w = std::max(w, th + gap + text_width(legend_label[first + j], sc));
        }
        note(n_bands + 1 + k, x, y, w, (n + 1) * (th + gap) - gap);
        first += n;
    }
}

// The tanglegram's text over the device canvas (ldw_plot_tng.hip): label k read UPWARDS from its anchor — the bottom-left corner of the turned text, 7
// scale pixels wide and text_width high — and the title centred at the top.  The anchors are the caller's layout; nothing is moved or left out here.
// boxes (may be NULL): x, y, w, h of the labels in their order, then of the title (w = 0: an empty string, nothing drawn); a box may reach past the canvas.
void plot_tng_overlay(uint8_t *canvas, int W, int H, const int32_t *label_xy, const char *const *labels, int n_labels, const char *title, int sc,
                      int32_t *boxes) {
    Canvas cv{canvas, W, H};
    auto note = [&](int k, int x, int y, int w, int h) {
        if (!boxes) return;
        boxes[4 * k] = x;
        boxes[4 * k + 1] = y;
        boxes[4 * k + 2] = w;
        boxes[4 * k + 3] = h;
    };
    for (int k = 0; k < n_labels; ++k) {
        const int x = label_xy[2 * k], y = label_xy[2 * k + 1], tw = text_width(labels[k], sc);
        if (tw == 0) {
            note(k, x, y, 0, 0);
            continue;
        }
        draw_text(cv, x, y, labels[k], sc, PLOT_TEXT, 1);
        note(k, x, y - tw + 1, 7 * sc, tw);
    }
    if (title && title[0]) {
        const int st = sc + sc / 2, tw = text_width(title, st);
        const int x = (W - tw) / 2, y = 2 * sc;
        draw_text(cv, x, y, title, st, PLOT_TITLE);
        note(n_labels, x, y, tw, 7 * st);
    } else {
        note(n_labels, 0, 0, 0, 0);
    }
}

}  // namespace ldw

using namespace ldw;

extern "C" {

int ldw_plot_ticks(double lo, double hi, int npx, int flip, double lim_out[2], double *tick_out, int32_t *px_out, int32_t *n_out) {
    LDW_REQUIRE(lim_out && tick_out && px_out && n_out, LDW_ERR_ARG, "ldw_plot_ticks: null argument");
    LDW_REQUIRE(npx >= 1, LDW_ERR_ARG, "ldw_plot_ticks: npx %d < 1", npx);
    LDW_REQUIRE(std::isfinite(lo) && std::isfinite(hi) && lo <= hi, LDW_ERR_ARG, "ldw_plot_ticks: the range [%g, %g] is not a finite interval", lo, hi);
    LDW_REQUIRE(plot_axis(lo, hi, npx, flip, lim_out, tick_out, px_out, n_out) == LDW_OK, LDW_ERR_ARG,
                "ldw_plot_ticks: the axis range of [%g, %g] is not finite", lo, hi);
    return LDW_OK;
}

// the tail of a layout: the data ranges are finite intervals, then both axes of the panel
static int layout_axes(ldw_plot_layout &L, double x_min, double x_max, double y_min, double y_max, const char *who) {
    LDW_REQUIRE(std::isfinite(x_min) && std::isfinite(x_max) && x_min <= x_max && std::isfinite(y_min) && std::isfinite(y_max) && y_min <= y_max,
                LDW_ERR_ARG, "%s: the data ranges are not finite intervals", who);
    LDW_REQUIRE(plot_axis(x_min, x_max, L.panel_w, 0, L.xlim, L.xtick, L.xtick_px, &L.n_xticks) == LDW_OK &&
                    plot_axis(y_min, y_max, L.panel_h, 1, L.ylim, L.ytick, L.ytick_px, &L.n_yticks) == LDW_OK,
                LDW_ERR_ARG, "%s: the axis range of the data is not finite", who);
    return LDW_OK;
}

int ldw_plot_layout_get(int kind, int n_panels, double x_min, double x_max, double y_min, double y_max, ldw_plot_layout *out) {
    LDW_REQUIRE(out, LDW_ERR_ARG, "ldw_plot_layout_get: null output");
    LDW_REQUIRE(kind >= LDW_PLOT_SR_CLUST && kind <= LDW_PLOT_LDMAP, LDW_ERR_ARG, "ldw_plot_layout_get: unknown figure kind %d", kind);
    LDW_REQUIRE(n_panels >= 1 && n_panels <= LDW_PLOT_MAX_PANELS && (kind == LDW_PLOT_SR_CLUST || n_panels == 1), LDW_ERR_ARG,
                "ldw_plot_layout_get: %d panels (1..%d for the facet figure, 1 otherwise)", n_panels, LDW_PLOT_MAX_PANELS);
    ldw_plot_layout &L = *out;
    memset(&L, 0, sizeof(L));
    L.n_panels = n_panels;
    if (kind == LDW_PLOT_LDMAP) {
        L.width = 5000;
        L.height = 5250;
        L.rows = L.cols = 1;
        L.panel_w = L.panel_h = 4600;
        L.panel[0][0] = 200;
        L.panel[0][1] = 450;
        L.panel[0][2] = L.panel[0][3] = 4600;
        return LDW_OK;
    }
    static const int R[11] = {0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 3}, Cc[11] = {0, 1, 2, 3, 2, 3, 3, 3, 3, 3, 4};   // ggplot2::wrap_dims
    L.width = kind == LDW_PLOT_LR ? 4800 : 2200;
    L.height = 1200;
    L.rows = R[n_panels];
    L.cols = Cc[n_panels];
    const bool cbar = kind != LDW_PLOT_LR, strips = kind == LDW_PLOT_SR_CLUST;
    const int left = 190, top = 30, bottom = 130, right = cbar ? 270 : 40, gap = 30, strip_h = strips ? 40 : 0;
    const int cell_w = (L.width - left - right - (L.cols - 1) * gap) / L.cols;
    const int cell_h = (L.height - top - bottom - (L.rows - 1) * gap) / L.rows;
    L.panel_w = cell_w;
    L.panel_h = cell_h - strip_h - (strips ? 1 : 0);
    for (int p = 0; p < n_panels; ++p) {
        const int r = p / L.cols, c = p % L.cols;
        const int x = left + c * (cell_w + gap), y = top + r * (cell_h + gap);
        L.panel[p][0] = x;
        L.panel[p][1] = y + strip_h + (strips ? 1 : 0);
        L.panel[p][2] = L.panel_w;
        L.panel[p][3] = L.panel_h;
        if (strips) {
            L.strip[p][0] = x - 1;
            L.strip[p][1] = y - 1;
            L.strip[p][2] = cell_w + 2;
            L.strip[p][3] = strip_h + 1;
        }
    }
    if (cbar) {
        L.cbar[2] = 50;
        L.cbar[3] = 400;
        L.cbar[0] = L.width - right + 50;
        L.cbar[1] = (L.height - 400) / 2;
    }
    return layout_axes(L, x_min, x_max, y_min, y_max, "ldw_plot_layout_get");
}

int ldw_plot_xy_layout_get(int kind, int n_panels, double x_min, double x_max, double y_min, double y_max, ldw_plot_layout *out) {
    LDW_REQUIRE(out, LDW_ERR_ARG, "ldw_plot_xy_layout_get: null output");
    LDW_REQUIRE(kind == LDW_PLOT_FIT || kind == LDW_PLOT_CDS, LDW_ERR_ARG, "ldw_plot_xy_layout_get: figure kind %d is no xy figure", kind);
    LDW_REQUIRE(n_panels == 1, LDW_ERR_ARG, "ldw_plot_xy_layout_get: %d panels (an xy figure has one)", n_panels);
    ldw_plot_layout &L = *out;
    memset(&L, 0, sizeof(L));
    L.n_panels = L.rows = L.cols = 1;
    L.width = 2200;
    L.height = 1200;
    const int left = 190, bottom = 130, top = kind == LDW_PLOT_FIT ? 70 : 30, right = kind == LDW_PLOT_CDS ? 270 : 40;
    L.panel_w = L.width - left - right;
    L.panel_h = L.height - top - bottom;
    L.panel[0][0] = left;
    L.panel[0][1] = top;
    L.panel[0][2] = L.panel_w;
    L.panel[0][3] = L.panel_h;
    return layout_axes(L, x_min, x_max, y_min, y_max, "ldw_plot_xy_layout_get");
}

int ldw_png_write(const char *path, const uint8_t *rgb, int32_t width, int32_t height, int level, int64_t *bytes_out) {
    LDW_REQUIRE(path && rgb, LDW_ERR_ARG, "ldw_png_write: null argument");
    LDW_REQUIRE(width >= 1 && height >= 1 && (int64_t)width * 3 + 1 < (1ll << 31), LDW_ERR_ARG, "ldw_png_write: %d x %d pixels", width, height);
    LDW_REQUIRE(level >= -1 && level <= 9, LDW_ERR_ARG, "ldw_png_write: compression level %d outside -1..9", level);
    FILE *f = fopen(path, "wb");
    LDW_REQUIRE(f, LDW_ERR_ARG, "ldw_png_write: cannot open %s for writing", path);
    int64_t total = 0;
    bool ok = true;
    auto be32 = [](uint8_t *p, uint32_t v) {
        p[0] = (uint8_t)(v >> 24);
        p[1] = (uint8_t)(v >> 16);
        p[2] = (uint8_t)(v >> 8);
        p[3] = (uint8_t)v;
    };
    auto chunk = [&](const char *type, const uint8_t *data, uint32_t len) {
        uint8_t head[8], tail[4];
        be32(head, len);
        memcpy(head + 4, type, 4);
        uint32_t crc = (uint32_t)crc32(0, head + 4, 4);
        if (len) crc = (uint32_t)crc32(crc, data, len);
        be32(tail, crc);
        ok = ok && fwrite(head, 1, 8, f) == 8 && (len == 0 || fwrite(data, 1, len, f) == len) && fwrite(tail, 1, 4, f) == 4;
        total += 12 + (int64_t)len;
    };
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    ok = fwrite(sig, 1, 8, f) == 8;
    total += 8;
    uint8_t ihdr[13];
    be32(ihdr, (uint32_t)width);
    be32(ihdr + 4, (uint32_t)height);
    ihdr[8] = 8;    // bit depth
    ihdr[9] = 2;    // colour type: RGB
    ihdr[10] = 0;   // deflate
    ihdr[11] = 0;   // adaptive filtering (every row uses filter 0)
    ihdr[12] = 0;   // not interlaced
    chunk("IHDR", ihdr, 13);
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (deflateInit(&zs, level < 0 ? 1 : level) != Z_OK) {
        fclose(f);
        remove(path);
        LDW_REQUIRE(false, LDW_ERR_ARG, "ldw_png_write: deflateInit failed");
    }
    const size_t stride = (size_t)width * 3;
    std::vector<uint8_t> row(stride + 1), outb(1u << 20);
    zs.next_out = outb.data();
    zs.avail_out = (uInt)outb.size();
    for (int32_t j = 0; j <= height && ok; ++j) {
        const bool last = j == height;
        if (!last) {
            row[0] = 0;
            memcpy(row.data() + 1, rgb + (size_t)j * stride, stride);
            zs.next_in = row.data();
            zs.avail_in = (uInt)(stride + 1);
        }
        for (;;) {
            const int zr = deflate(&zs, last ? Z_FINISH : Z_NO_FLUSH);
            if (zr == Z_STREAM_ERROR) {
                ok = false;
                break;
            }
            if (zs.avail_out == 0 || (last && zr == Z_STREAM_END)) {
                const uint32_t have = (uint32_t)(outb.size() - zs.avail_out);
                if (have) chunk("IDAT", outb.data(), have);
                zs.next_out = outb.data();
                zs.avail_out = (uInt)outb.size();
            }
            if (last ? zr == Z_STREAM_END : zs.avail_in == 0) break;
        }
    }
    deflateEnd(&zs);
    chunk("IEND", nullptr, 0);
    ok = (fclose(f) == 0) && ok;
    if (!ok) remove(path);   // no truncated picture is left behind
    LDW_REQUIRE(ok, LDW_ERR_ARG, "ldw_png_write: writing %s failed", path);
    if (bytes_out) *bytes_out = total;
    return LDW_OK;
}

int ldw_debug_plot_colours(int kind, const double *t, int64_t n, uint8_t *rgb_out) {
    LDW_REQUIRE(rgb_out && (kind == 0 || (kind == 1 && n >= 0 && (t || n == 0))), LDW_ERR_ARG, "ldw_debug_plot_colours: bad argument");
    if (kind == 0) {
        plot_ramp_table(rgb_out);
        return LDW_OK;
    }
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t c = plot_gradient(t[i]);
        rgb_out[i * 3] = (uint8_t)(c >> 16);
        rgb_out[i * 3 + 1] = (uint8_t)(c >> 8);
        rgb_out[i * 3 + 2] = (uint8_t)c;
    }
    return LDW_OK;
}

}  // extern "C"
