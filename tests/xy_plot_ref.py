"""A NAIVE painter of the xy figures ("xy"), in numpy and 64-bit integers, written from the rules and not from the HIP code:
one point after the other in row order, then one segment after the other, each over its bounding box."""
import numpy as np

import plot_ref as R

MAX_VERTS = 1 << 17


def finite_vertices(lx, ly):
    lx, ly = np.asarray(lx, dtype=np.float64), np.asarray(ly, dtype=np.float64)
    return np.isfinite(lx) & np.isfinite(ly)


def data_ranges(x, y, lx=(), ly=()):
    """((x min, x max), (y min, y max)) of the kept points and the finite line vertices together; the unit ranges when there are none."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    k = np.isfinite(x) & np.isfinite(y)
    f = finite_vertices(lx, ly)
    ax = np.concatenate([x[k], np.asarray(lx, dtype=np.float64)[f]])
    ay = np.concatenate([y[k], np.asarray(ly, dtype=np.float64)[f]])
    if len(ax) == 0:
        return (0.0, 1.0), (0.0, 1.0)
    return (ax.min(), ax.max()), (ay.min(), ay.max())


def covers(x0, y0, x1, y1, w, px, py):
    """The network plot's rule, 4 D2 <= w^2 with D2 the squared distance from the pixel to the segment, in 64-bit integers (px, py: int64 arrays;
    panels up to 8192 pixels and w up to 1024 keep every product below 2^62)."""
    qx, qy, dx, dy = px - x0, py - y0, x1 - x0, y1 - y0
    dd, t = dx * dx + dy * dy, qx * dx + qy * dy
    cr = qx * dy - qy * dx
    return np.where(t <= 0, 4 * (qx * qx + qy * qy) <= w * w,
                    np.where(t >= dd, 4 * ((qx - dx) ** 2 + (qy - dy) ** 2) <= w * w, 4 * cr * cr <= w * w * dd))


def segments(lx, ly, x0, x1, y0, y1, W, H):
    """The pixel segments of the polyline, in vertex order: (ax, ay, bx, by); an isolated finite vertex gives (ax, ay, ax, ay)."""
    f = finite_vertices(lx, ly)
    n = len(f)
    if n == 0:
        return []
    px = R.pixel(np.where(f, lx, x0), x0, x1, W)
    py = H - 1 - R.pixel(np.where(f, ly, y0), y0, y1, H)
    out = []
    for i in range(n):
        if not f[i]:
            continue
        if i + 1 < n and f[i + 1]:
            out.append((int(px[i]), int(py[i]), int(px[i + 1]), int(py[i + 1])))
        elif not (i > 0 and f[i - 1]):
            out.append((int(px[i]), int(py[i]), int(px[i]), int(py[i])))
    return out


def paint(x, y, cls, n_classes, class_rgb, W, H, D, xtick_px, ytick_px, lx=(), ly=(), line_w=5, line_rgb=0xFF0000, ranges=None):
    """((H, W, 3) uint8, rows dropped).  ValueError where the library refuses: a class >= n_classes, more than 2^17 vertices."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = len(x)
    cls = np.zeros(n, dtype=np.int64) if cls is None else np.asarray(cls).astype(np.int64)
    lx, ly = np.asarray(lx, dtype=np.float64), np.asarray(ly, dtype=np.float64)
    if (cls >= n_classes).any():
        raise ValueError("class out of range")
    if len(lx) > MAX_VERTS:
        raise ValueError("too many vertices")
    keep = np.isfinite(x) & np.isfinite(y)
    xr, yr = data_ranges(x, y, lx, ly) if ranges is None else ranges
    x0, x1 = R.axis_range(*xr)
    y0, y1 = R.axis_range(*yr)
    img = np.empty((H, W, 3), dtype=np.uint8)
    img[:] = R.BG
    img[:, np.asarray(xtick_px, dtype=np.int64)] = R.GRID
    img[np.asarray(ytick_px, dtype=np.int64)] = R.GRID
    rows = np.flatnonzero(keep)
    if len(rows):
        px = R.pixel(x[rows], x0, x1, W)
        py = H - 1 - R.pixel(y[rows], y0, y1, H)
        off = np.array(R.disc_offsets(D), dtype=np.int64)
        col = np.array([R.rgb_of(int(c)) for c in class_rgb], dtype=np.uint8)[cls[rows]]
        flat = img.reshape(-1, 3)
        for a in range(0, len(rows), 100_000):       # row-major (row, offset): numpy assigns repeated indices in order, so the later row wins
            b = min(a + 100_000, len(rows))
            qx = px[a:b, None] + off[None, :, 0]
            qy = py[a:b, None] + off[None, :, 1]
            ok = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            flat[(qy * W + qx)[ok]] = np.broadcast_to(col[a:b, None, :], (b - a, len(off), 3))[ok]
    r = (line_w + 1) // 2
    lc = R.rgb_of(int(line_rgb))
    done = set()
    for seg in segments(lx, ly, x0, x1, y0, y1, W, H):
        if seg in done:                                  # (opaque and of one colour: a repeated segment paints the same pixels again)
            continue
        done.add(seg)
        ax, ay, bx, by = seg
        ya, yb = max(min(ay, by) - r, 0), min(max(ay, by) + r, H - 1)
        xa, xb = max(min(ax, bx) - r, 0), min(max(ax, bx) + r, W - 1)
        qy, qx = np.mgrid[ya:yb + 1, xa:xb + 1].astype(np.int64)
        img[ya:yb + 1, xa:xb + 1][covers(ax, ay, bx, by, line_w, qx, qy)] = lc
    return img, int(n - keep.sum())
