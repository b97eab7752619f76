"""The device side of the xy figures (ldweaver_amd/csrc/ldw_plot_xy.hip, DESIGN.md 20 "xy") against the naive painter of xy_plot_ref.py: every
pixel of the panel must equal the painter's.  The panel is 97 x 70 pixels — no multiple of the 32-pixel tile.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest

import plot_ref as R
import xy_plot_ref as X
from ldweaver_amd import _lib as L
from ldweaver_amd import plots as P

pytestmark = pytest.mark.gpu

W, H = 97, 70
PAL = [0x000000, 0xF8766D, 0x00BA38, 0x619CFF, 0x111111, 0x222222, 0x333333, 0x444444, 0x555555, 0xABCDEF]


def reference(x, y, cls, n_classes, D, line=None, line_w=5, line_rgb=0xFF0000, w=W, h=H, pal=PAL):
    lx, ly = ((), ()) if line is None else line
    xr, yr = X.data_ranges(x, y, lx, ly)
    _, _, xt = P.ticks(xr[0], xr[1], w, False)
    _, _, yt = P.ticks(yr[0], yr[1], h, True)
    return X.paint(x, y, cls, n_classes, pal[:n_classes], w, h, D, xt, yt, lx, ly, line_w, line_rgb)


def render(engine, x, y, cls, n_classes, D, line=None, line_w=5, line_rgb=0xFF0000, w=W, h=H, pal=PAL):
    o = P.xy_opts(L.PLOT_CDS, D, pal[:n_classes], line_w, line_rgb)
    img, st, _ = P.debug_xy_panel(engine, x, y, cls, line, opts=o, W=w, H=h)
    return img, st


def check(engine, x, y, cls, n_classes, D, **kw):
    want, dropped = reference(x, y, cls, n_classes, D, **kw)
    got, st = render(engine, x, y, cls, n_classes, D, **kw)
    assert np.array_equal(got, want), f"{int((got != want).any(axis=2).sum())} pixels differ"
    assert st["dropped"] == dropped and st["kept"] == len(x) - dropped
    return got


def cloud(n, n_classes, seed):
    rng = np.random.default_rng(seed)
    return np.floor(rng.random(n) * 5000.0), rng.random(n) ** 2, rng.integers(0, n_classes, n).astype(np.uint8)


@pytest.mark.parametrize("D", [1, 11, 41])
def test_points_equal_the_painter(engine, D):
    x, y, cls = cloud(300, 3, D)
    img = check(engine, x, y, cls, 3, D)
    assert {R.rgb_of(c) for c in PAL[:3]} <= {tuple(int(v) for v in p) for p in img.reshape(-1, 3)}      # the three classes are all seen
    # the four corners and the middles of the four edges: discs clipped at the panel
    ex = np.array([0.0, 0.0, 1.0, 1.0, 0.5, 0.5, 0.0, 1.0])
    ey = np.array([0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.5, 0.5])
    # (the axis range is widened by 5 %, so the extreme rows sit in from the border by less than a large disc's radius)
    check(engine, ex, ey, np.arange(8, dtype=np.uint8) % 3, 3, D)


@pytest.mark.parametrize("k", [2, 3])
def test_later_row_wins_where_discs_overlap(engine, k):
    x = np.array([10.0, 11.0, 12.0, 0.0, 100.0])[[0, 1, 2][:k] + [3, 4]]
    y = np.array([5.0, 5.2, 5.1, 0.0, 10.0])[[0, 1, 2][:k] + [3, 4]]
    cls = np.array([1, 2, 3, 0, 0], dtype=np.uint8)[[0, 1, 2][:k] + [3, 4]]
    a = check(engine, x, y, cls, 4, 11)
    order = np.r_[np.arange(k)[::-1], k, k + 1]
    b = check(engine, x[order], y[order], cls[order], 4, 11)
    assert not np.array_equal(a, b)                                      # swapping the rows changes the picture
    top = R.rgb_of(PAL[int(cls[k - 1])])
    px, py = int(R.pixel(x[k - 1], *R.axis_range(0.0, 100.0), W)), H - 1 - int(R.pixel(y[k - 1], *R.axis_range(0.0, 10.0), H))
    assert tuple(a[py, px]) == top


def test_classes(engine):
    x, y, cls = cloud(200, 10, 3)
    cls[:2] = (0, 9)
    check(engine, x, y, cls, 10, 11)
    got_null, _ = render(engine, x, y, None, 10, 11)                     # cls == NULL: class 0
    assert np.array_equal(got_null, reference(x, y, np.zeros(len(x), dtype=np.uint8), 10, 11)[0])
    bad = cls.copy()
    bad[17] = 10
    with pytest.raises(L.LdwError) as e:
        render(engine, x, y, bad, 10, 11)
    assert e.value.code == L.LDW_ERR_ARG and "class" in str(e.value)
    bad = np.zeros(len(x), dtype=np.uint8)
    bad[5], xx = 3, x.copy()
    xx[5] = np.nan                                                       # a dropped row's class counts too
    with pytest.raises(L.LdwError):
        render(engine, xx, y, bad, 3, 11)


def test_empty_single_and_dropped_rows(engine):
    z = np.zeros(0)
    img = check(engine, z, z, None, 1, 11)
    assert {tuple(p) for p in img.reshape(-1, 3)} == {R.BG, R.GRID}     # a white panel with grid lines over [0, 1]
    img = check(engine, np.array([3.0]), np.array([-2.0]), np.array([1], dtype=np.uint8), 2, 11)      # zero-width ranges
    assert (img == np.array(R.rgb_of(PAL[1]), dtype=np.uint8)).all(axis=2).sum() == len(R.disc_offsets(11))
    x, y, cls = cloud(64, 2, 9)
    x[3], x[10], y[11], y[40], x[41] = np.nan, np.inf, -np.inf, np.nan, -np.inf
    y[3] = np.nan
    _, st = render(engine, x, y, cls, 2, 11)
    assert st["dropped"] == 5
    check(engine, x, y, cls, 2, 11)
    check(engine, np.full(4, np.nan), np.arange(4.0), None, 1, 11)       # every row dropped: the unit ranges


def test_host_chunks_carry_the_global_row(engine):
    """2^20 + 3 host rows, the last three over the first three: the second chunk's rows must beat the first's."""
    n = (1 << 20) + 3
    rng = np.random.default_rng(4)
    x, y = np.floor(rng.random(n) * 1000.0), np.floor(rng.random(n) * 1000.0)
    cls = rng.integers(0, 3, n).astype(np.uint8)
    x[:3], y[:3] = (10.0, 500.0, 990.0), (10.0, 500.0, 990.0)
    x[-3:], y[-3:] = x[:3], y[:3]
    cls[:3], cls[-3:] = 2, (1, 0, 1)
    x[3:-3] = np.where((np.abs(x[3:-3] - 500.0) < 30) & (np.abs(y[3:-3] - 500.0) < 40), 200.0, x[3:-3])      # keep the middle pixel clear of the crowd
    got = check(engine, x, y, cls, 3, 1)
    xl, yl = R.axis_range(x.min(), x.max()), R.axis_range(y.min(), y.max())
    assert tuple(got[H - 1 - int(R.pixel(500.0, *yl, H)), int(R.pixel(500.0, *xl, W))]) == R.rgb_of(PAL[0])      # row n - 2 (class 0) over row 1 (class 2)


def test_device_columns_give_the_same_bytes(engine):
    import torch
    x, y, cls = cloud(5000, 4, 12)
    x[5] = np.nan
    line = (np.linspace(0, 5000, 40), np.linspace(0.9, 0.1, 40))
    host, sh = render(engine, x, y, cls, 4, 11, line=line)
    dev = torch.device("cuda", engine.device)
    got, sd = render(engine, torch.as_tensor(x, device=dev), torch.as_tensor(y, device=dev), torch.as_tensor(cls, device=dev), 4, 11, line=line)
    assert np.array_equal(host, got) and sh == sd
    assert np.array_equal(host, reference(x, y, cls, 4, 11, line=line)[0])


# ---- the line -----------------------------------------------------------------------------------------------------------------------------------------

def _pts():
    return np.array([0.0, 100.0]), np.array([0.0, 10.0]), np.zeros(2, dtype=np.uint8)


@pytest.mark.parametrize("line_w", [1, 5, 12])
def test_line_shapes(engine, line_w):
    x, y, cls = _pts()
    nan = np.nan
    cases = {
        "none": (np.zeros(0), np.zeros(0)),
        "one vertex": (np.array([50.0]), np.array([5.0])),
        "two vertices": (np.array([10.0, 90.0]), np.array([2.0, 9.0])),
        "one pixel": (np.array([50.0, 50.2]), np.array([5.0, 5.01])),
        "vertical": (np.array([40.0, 40.0]), np.array([1.0, 9.0])),
        "horizontal": (np.array([5.0, 95.0]), np.array([6.0, 6.0])),
        "steep over the tile edges": (np.array([29.6, 34.1]), np.array([0.5, 9.5])),      # px 30 -> 34: crosses x = 31..33 over the whole height
        "clipped at the axis limits": (np.array([0.0, 100.0, 100.0]), np.array([10.0, 10.0, 0.0])),
        "broken by NaN": (np.array([10.0, 30.0, nan, 60.0, nan, nan, 80.0, 90.0, 70.0]), np.array([1.0, 8.0, 5.0, 5.0, nan, 2.0, nan, 3.0, 9.0])),
    }
    for name, line in cases.items():
        img = check(engine, x, y, cls, 1, 11, line=line, line_w=line_w, line_rgb=0x0000FF)
        red = int((img == np.array([0, 0, 255], dtype=np.uint8)).all(axis=2).sum())
        assert (red > 0) == (name != "none"), name
    segs = X.segments(*cases["broken by NaN"], *R.axis_range(0.0, 100.0), *R.axis_range(0.0, 10.0), W, H)
    assert len(segs) == 3 and segs[1][:2] == segs[1][2:] and segs[0][:2] != segs[0][2:]      # a segment, an isolated vertex (60, 5), nothing, the segment 90-70


def test_noisy_decay_curve_and_line_over_points(engine):
    rng = np.random.default_rng(8)
    n = 3000
    ln = np.arange(1.0, n + 1)
    mx = 0.4 * np.exp(-ln / 700.0) + 0.02 + rng.normal(0, 0.004, n)
    fit = 0.4 * np.exp(-ln / 700.0) + 0.02
    img = check(engine, ln, mx, None, 1, 11, line=(ln, mx), line_w=1)     # 3000 vertices on 97 columns: most segments are degenerate
    img = check(engine, ln, mx, None, 1, 11, line=(ln, fit), line_w=5)
    # a pixel under both a point and the line shows the line
    xl, yl = R.axis_range(1.0, float(n)), R.axis_range(float(min(mx.min(), fit.min())), float(max(mx.max(), fit.max())))
    px, py = int(R.pixel(ln[1500], *xl, W)), H - 1 - int(R.pixel(fit[1500], *yl, H))
    assert tuple(img[py, px]) == (255, 0, 0)
    pts_only, _ = render(engine, ln, mx, None, 1, 11)
    assert tuple(pts_only[py, px]) == (0, 0, 0)


def test_vertex_limit(engine):
    x, y, cls = _pts()
    n = 1 << 17
    lx = np.linspace(0.0, 100.0, n)
    ly = 5.0 + 4.0 * np.sin(lx / 7.0)
    check(engine, x, y, cls, 1, 11, line=(lx, ly), line_w=5)
    with pytest.raises(L.LdwError) as e:
        render(engine, x, y, cls, 1, 11, line=(np.r_[lx, 1.0], np.r_[ly, 1.0]))
    assert e.value.code == L.LDW_ERR_ARG and "vertices" in str(e.value)


def test_refusals_come_before_anything_runs(engine):
    lib = L.lib()
    x = np.arange(4.0)
    rgb = np.zeros((H, W, 3), dtype=np.uint8)

    def call(o, xp=x, yp=x, n=4, lx=None, ly=None, nl=0, w=W, h=H, out=rgb):
        return lib.ldw_debug_plot_xy_panel(engine._ctx, L.ptr(xp), L.ptr(yp), None, n, 0, L.ptr(lx), L.ptr(ly), nl, None if o is None else C.byref(o), w, h,
                                           L.ptr(out), None, None)

    assert call(P.xy_opts(L.PLOT_CDS)) == L.LDW_OK
    assert call(None) == L.LDW_ERR_ARG
    assert call(P.xy_opts(L.PLOT_CDS), xp=None) == L.LDW_ERR_ARG and call(P.xy_opts(L.PLOT_CDS), yp=None) == L.LDW_ERR_ARG      # null columns with n > 0
    assert call(P.xy_opts(L.PLOT_CDS), xp=None, yp=None, n=0) == L.LDW_OK
    for D in (2, 43, -1):
        assert call(P.xy_opts(L.PLOT_CDS, D)) == L.LDW_ERR_ARG, D
    for nc in (0, 11):
        o = P.xy_opts(L.PLOT_CDS)
        o.n_classes = nc
        assert call(o) == L.LDW_ERR_ARG, nc
    assert call(P.xy_opts(L.PLOT_CDS, line_w=1025)) == L.LDW_ERR_ARG and call(P.xy_opts(L.PLOT_CDS, line_w=-1)) == L.LDW_ERR_ARG
    assert call(P.xy_opts(L.PLOT_CDS, line_rgb=0x1000000)) == L.LDW_ERR_ARG
    assert call(P.xy_opts(L.PLOT_CDS, class_rgb=[0x1000000])) == L.LDW_ERR_ARG
    assert call(P.xy_opts(L.PLOT_SR_COMBI)) == L.LDW_ERR_ARG and call(P.xy_opts(6)) == L.LDW_ERR_ARG
    assert call(P.xy_opts(L.PLOT_CDS), nl=2) == L.LDW_ERR_ARG                      # vertices announced, none given
    assert call(P.xy_opts(L.PLOT_CDS), w=0) == L.LDW_ERR_ARG and call(P.xy_opts(L.PLOT_CDS), h=8193) == L.LDW_ERR_ARG
    assert call(P.xy_opts(L.PLOT_CDS), out=None) == L.LDW_ERR_ARG
    o = P.xy_opts(L.PLOT_FIT)
    assert lib.ldw_plot_xy(engine._ctx, L.ptr(x), L.ptr(x), None, 4, 0, None, None, 0, C.byref(o), None, None, None, None, None, None) == L.LDW_ERR_ARG
    # the defaults: D = 0 is 11, line_w = 0 is 5
    a, _ = render(engine, x, x, None, 1, 0, line=(x, x[::-1].copy()), line_w=0)
    assert np.array_equal(a, reference(x, x, None, 1, 11, line=(x, x[::-1].copy()), line_w=5)[0])


# ---- through the public calls ----------------------------------------------------------------------------------------------------------------------------

def _figure_checks(path, kind, x, y, cls, n_classes, pal, line):
    img, ihdr = R.png_decode(open(path, "rb").read())
    assert img.shape == (1200, 2200, 3)
    lx, ly = ((), ()) if line is None else line
    lay = P.layout(kind, 1, *X.data_ranges(x, y, lx, ly))
    px, py, pw, ph = lay["panels"][0]
    want, _ = X.paint(x, y, cls, n_classes, pal, pw, ph, 11, lay["xtick_px"], lay["ytick_px"], lx, ly, 5, P.FIT_LINE)
    assert np.array_equal(img[py:py + ph, px:px + pw], want)
    outside = img.copy()
    outside[py:py + ph, px:px + pw] = 255
    assert (outside != 255).any()                                       # the frame and the text are drawn
    return img


def test_fit_plot_and_cds_cluster_plot(engine, tmp_path):
    import pandas as pd
    from ldweaver_amd.network import hue_palette
    from ldweaver_amd.snpdat import CdsVar
    rng = np.random.default_rng(21)
    ln = np.arange(1.0, 20000.0, 67.0)
    fd = pd.DataFrame({"len": ln, "max": 0.3 * np.exp(-ln / 4000.0) + 0.03 + rng.normal(0, 0.005, len(ln)), "fit": 0.3 * np.exp(-ln / 4000.0) + 0.03})
    p1, p2 = str(tmp_path / "c2_fit.png"), str(tmp_path / "c2_fit_again.png")
    assert P.fit_plot(fd, 2, p1, engine=engine) == p1
    P.fit_plot(fd, 2, p2, engine=engine)
    assert open(p1, "rb").read() == open(p2, "rb").read()
    a = _figure_checks(p1, L.PLOT_FIT, fd["len"].to_numpy(), fd["max"].to_numpy(), None, 1, [0], (fd["len"].to_numpy(), fd["fit"].to_numpy()))
    P.fit_plot(fd, 3, p2, engine=engine)                                # the title is part of the picture
    assert not np.array_equal(a, R.png_decode(open(p2, "rb").read())[0])

    n = 900
    start = np.sort(rng.integers(1, 2_000_000, n))
    var = rng.random(n) ** 3
    lab = (1 + (var > 0.1) + (var > 0.5)).astype(np.int32)
    cv = CdsVar(paint=np.ones(3, dtype=np.int32), nclust=3, var_estimate=var, cds_start=start, cds_end=start + 900, clusts={"km_clst_ord": lab, "cutoff": 0.1})
    q1, q2 = str(tmp_path / "CDS_clustering.png"), str(tmp_path / "CDS_again.png")
    P.cds_cluster_plot(cv, q1, engine=engine)
    P.cds_cluster_plot(cv, q2, engine=engine)
    assert open(q1, "rb").read() == open(q2, "rb").read()
    pal = [int(c) for c in hue_palette(3)]
    img = _figure_checks(q1, L.PLOT_CDS, start.astype(np.float64), var, (lab - 1).astype(np.uint8), 3, pal, None)
    seen = {tuple(p) for p in img[:, 1940:].reshape(-1, 3)}
    assert {R.rgb_of(c) for c in pal} <= seen                           # the legend's swatches right of the panel
    with pytest.raises(ValueError):
        P.cds_cluster_plot(CdsVar(paint=np.ones(3), nclust=11, var_estimate=var, cds_start=start, cds_end=start, clusts={"km_clst_ord": lab, "cutoff": 0}), q2,
                           engine=engine)
