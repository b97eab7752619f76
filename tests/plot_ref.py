"""numpy restatement of the plot rules, written from the rules and not from the HIP code: the axis range and the pixel rule,
the scatter gradient, the LD map's ramp, a NAIVE painter that stamps every point's disc in the reference's draw order (last write wins),
and a small PNG decoder (zlib, all five filter types) so that no imaging library is needed."""
import struct
import zlib

import numpy as np

BG, GRID, GREY = (255, 255, 255), (0xEB, 0xEB, 0xEB), (0xC0, 0xC0, 0xC0)
STOPS = np.array([[0x45, 0x75, 0xB4], [0x91, 0xBF, 0xDB], [0xE0, 0xF3, 0xF8], [0xFE, 0xE0, 0x90], [0xFC, 0x8D, 0x59], [0xD7, 0x30, 0x27]], dtype=np.float64)
RAMP_STOPS = np.array([[0xFF, 0xFF, 0xFF], [0xE1, 0xB9, 0xB4], [0xAE, 0x45, 0x2C], [0x80, 0x24, 0x18]], dtype=np.float64)


def rgb_of(v: int):
    return ((v >> 16) & 255, (v >> 8) & 255, v & 255)


def axis_range(lo: float, hi: float):
    """Data range widened by 5 % on both sides; a zero-width range by +-0.5 first."""
    lo, hi = np.float64(lo), np.float64(hi)
    if hi == lo:
        lo, hi = lo - 0.5, hi + 0.5
    d = (hi - lo) * 0.05
    return lo - d, hi + d


def pixel(v, v0, v1, n: int):
    """min(n - 1, (int)floor((v - v0) / (v1 - v0) * n)), fp64."""
    v = np.asarray(v, dtype=np.float64)
    return np.minimum(n - 1, np.floor((v - v0) / (v1 - v0) * n).astype(np.int64))


def gradient(t):
    """rev(brewer.pal(6, "RdYlBu")), piecewise linear in sRGB, rounded half up: (n, 3) uint8."""
    t = np.asarray(t, dtype=np.float64)
    t5 = 5.0 * t
    s = np.minimum(np.floor(t5), 4).astype(np.int64)
    f = (t5 - s)[:, None]
    return np.floor(STOPS[s] + (STOPS[s + 1] - STOPS[s]) * f + 0.5).astype(np.uint8)


def ramp():
    """colorRampPalette(c("white", "#E1B9B4", "#AE452C", "#802418"))(2056): linear RGB, rounded half up."""
    p = 3.0 * (np.arange(2056, dtype=np.float64) / 2055.0)
    s = np.minimum(np.floor(p), 2).astype(np.int64)
    f = (p - s)[:, None]
    return np.floor(RAMP_STOPS[s] + (RAMP_STOPS[s + 1] - RAMP_STOPS[s]) * f + 0.5).astype(np.uint8)


def heat_raster(htm, W: int, H: int):
    """Nearest neighbour, row 0 at the bottom, palette index min(floor(v * 2056), 2055) (non-finite: 0)."""
    htm = np.asarray(htm, dtype=np.float64)
    B = htm.shape[0]
    r = ((H - 1 - np.arange(H, dtype=np.int64)) * B) // H
    c = (np.arange(W, dtype=np.int64) * B) // W
    v = htm[r][:, c]
    with np.errstate(invalid="ignore"):
        k = np.where(np.isfinite(v), np.clip(np.floor(v * 2056.0), 0, 2055), 0).astype(np.int64)
    return ramp()[k]


def disc_offsets(D: int):
    h = D // 2
    return [(dx, dy) for dy in range(-h, h + 1) for dx in range(-h, h + 1) if 4 * (dx * dx + dy * dy) <= D * D]


def keep_mask(x, y, srp=None):
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    k = np.isfinite(x) & np.isfinite(y)
    if srp is not None:
        s = np.asarray(srp, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            k &= np.isfinite(s) & (s >= 0)
    return k


def data_ranges(x, y, srp=None, hline=None):
    """((x min, x max), (y min, y max)) of the kept rows (unit ranges when none), the line's y included."""
    k = keep_mask(x, y, srp)
    x, y = np.asarray(x, dtype=np.float64)[k], np.asarray(y, dtype=np.float64)[k]
    xr = (x.min(), x.max()) if len(x) else (0.0, 1.0)
    yr = (y.min(), y.max()) if len(y) else (0.0, 1.0)
    if hline is not None:
        yr = (min(yr[0], hline), max(yr[1], hline)) if len(y) else (hline, hline)
    return xr, yr


def draw_order(srp, layer, ordered: bool):
    """Indices of the rows in the order ggplot draws them: sr_links[order(srp_max, decreasing = T), ] unless ordered, reversed, the
    ARACNE == 0 rows before the ARACNE == 1 rows (R/prepareGWESplots.R:96-106)."""
    n = len(layer)
    idx = np.arange(n) if (ordered or srp is None) else np.argsort(-np.asarray(srp, dtype=np.float64), kind="stable")
    idx = idx[::-1]
    lay = np.asarray(layer)[idx] != 0
    return np.concatenate([idx[~lay], idx[lay]])


def naive_painter(x, y, srp, layer, panel, n_panels: int, W: int, H: int, D: int, ordered: bool, xtick_px, ytick_px, layer_rgb=None, hline=None,
                  hline_rgb=None, chunk: int = 100_000, ranges=None, srp_range=None):
    """(n_panels, H, W, 3) uint8: every kept row's disc stamped in draw order, clipped at the panel, over the white panel with its grid
    lines; the line (if any) over everything.  layer_rgb (two 0xRRGGBB): fixed colours instead of grey / gradient of srp.
    ranges = ((x min, x max), (y min, y max)) / srp_range = (lo, hi): those of a larger table of which the rows given are a part."""
    n = len(x)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    layer = np.ones(n, dtype=np.uint8) if layer is None else (np.asarray(layer) != 0).astype(np.uint8)
    panel = np.zeros(n, dtype=np.int64) if panel is None else np.asarray(panel).astype(np.int64)
    s = None if srp is None else np.where(np.asarray(srp, dtype=np.float64) == 0, 0.0, np.asarray(srp, dtype=np.float64))
    keep = keep_mask(x, y, s)
    xr, yr = data_ranges(x, y, s, hline) if ranges is None else ranges
    x0, x1 = axis_range(*xr)
    y0, y1 = axis_range(*yr)
    img = np.empty((n_panels, H, W, 3), dtype=np.uint8)
    img[:] = BG
    img[:, :, np.asarray(xtick_px, dtype=np.int64)] = GRID
    img[:, np.asarray(ytick_px, dtype=np.int64)] = GRID
    order = draw_order(s, layer, ordered)
    order = order[keep[order]]
    if len(order):
        px = pixel(x[order], x0, x1, W)
        py = H - 1 - pixel(y[order], y0, y1, H)
        lay, pan = layer[order], panel[order]
        if layer_rgb is not None:
            col = np.array([rgb_of(layer_rgb[0]), rgb_of(layer_rgb[1])], dtype=np.uint8)[lay]
        else:
            col = np.empty((len(order), 3), dtype=np.uint8)
            col[:] = GREY
            if lay.any():
                s1 = s[order][lay != 0]
                lo, hi = (s1.min(), s1.max()) if srp_range is None else srp_range
                t = np.full(len(s1), 0.5) if hi == lo else (s1 - lo) / (hi - lo)
                col[lay != 0] = gradient(t)
        off = np.array(disc_offsets(D), dtype=np.int64)
        flat = img.reshape(-1, 3)
        for a in range(0, len(order), chunk):       # row-major (row, offset): numpy assigns repeated indices in order, the last one wins
            b = min(a + chunk, len(order))
            qx = px[a:b, None] + off[None, :, 0]
            qy = py[a:b, None] + off[None, :, 1]
            ok = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            at = ((pan[a:b, None] * H + qy) * W + qx)[ok]
            flat[at] = np.broadcast_to(col[a:b, None, :], (b - a, len(off), 3))[ok]
    if hline is not None:
        img[:, H - 1 - int(pixel(hline, y0, y1, H))] = rgb_of(hline_rgb)
    return img


def png_decode(data: bytes):
    """(rgb (H, W, 3) uint8, IHDR fields) of an 8-bit RGB non-interlaced PNG; every chunk's CRC is checked."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "signature"
    at, idat, ihdr, seen_end = 8, b"", None, False
    while at < len(data):
        n, typ = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == (zlib.crc32(typ + body) & 0xFFFFFFFF), f"CRC of {typ}"
        at += 12 + n
        if typ == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif typ == b"IDAT":
            idat += body
        elif typ == b"IEND":
            seen_end = True
    assert ihdr is not None and seen_end and at == len(data)
    W, H, depth, ctype, comp, filt, lace = ihdr
    assert (depth, ctype, comp, filt, lace) == (8, 2, 0, 0, 0), ihdr
    raw = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(H, 1 + 3 * W)
    out = np.zeros((H, 3 * W), dtype=np.uint8)
    for j in range(H):
        f, line = int(raw[j, 0]), raw[j, 1:].astype(np.int64)
        up = out[j - 1].astype(np.int64) if j else np.zeros(3 * W, dtype=np.int64)
        if f == 0:
            cur = line
        elif f == 2:
            cur = line + up
        else:   # 1 Sub, 3 Average, 4 Paeth: each byte needs the one three to its left
            cur = np.zeros(3 * W, dtype=np.int64)
            for i in range(3 * W):
                a = cur[i - 3] if i >= 3 else 0
                b, c = up[i], (up[i - 3] if i >= 3 else 0)
                if f == 1:
                    pred = a
                elif f == 3:
                    pred = (a + b) // 2
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[i] = (line[i] + pred) & 255
        out[j] = cur & 255
    return out.reshape(H, W, 3), ihdr
