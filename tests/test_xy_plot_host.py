"""The host side of the xy figures ("xy"): the layouts of c<i>_fit.png and CDS_clustering.png, the naive painter of
xy_plot_ref.py against plot_ref's where the two rule sets coincide, and the refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

import plot_ref as R
import xy_plot_ref as X
from ldweaver_amd import _lib as L
from ldweaver_amd import plots as P


@pytest.mark.parametrize("kind", [L.PLOT_FIT, L.PLOT_CDS])
def test_layouts_of_the_xy_figures(kind):
    lay = P.layout(kind, 1, (1.0, 19999.0), (0.001, 0.3))
    assert (lay["width"], lay["height"]) == (2200, 1200) == P.CANVAS[kind]
    assert lay["n_panels"] == 1 and (lay["rows"], lay["cols"]) == (1, 1) and not lay["strips"] and lay["cbar"] is None
    x, y, w, h = lay["panels"][0]
    assert (w, h) == (lay["panel_w"], lay["panel_h"]) and x > 0 and y > 0 and x + w < 2200 and y + h < 1200
    if kind == L.PLOT_FIT:
        assert y >= 7 * 4 + 8                      # room for the title above the panel
    else:
        assert 2200 - (x + w) >= 200               # room for the legend right of it
    want = R.axis_range(1.0, 19999.0), R.axis_range(0.001, 0.3)
    assert lay["xlim"] == tuple(float(v) for v in want[0]) and lay["ylim"] == tuple(float(v) for v in want[1])
    assert np.array_equal(lay["xtick_px"], R.pixel(lay["xticks"], *lay["xlim"], w))
    assert np.array_equal(lay["ytick_px"], h - 1 - R.pixel(lay["yticks"], *lay["ylim"], h))
    with pytest.raises(L.LdwError):
        P.layout(kind, 2)
    lib, out = L.lib(), L.PlotLayout()
    assert lib.ldw_plot_xy_layout_get(kind, 1, 0.0, 1.0, 0.0, 1.0, None) == L.LDW_ERR_ARG
    assert lib.ldw_plot_xy_layout_get(kind, 1, 0.0, float("nan"), 0.0, 1.0, C.byref(out)) == L.LDW_ERR_ARG
    assert lib.ldw_plot_xy_layout_get(kind, 1, 2.0, 1.0, 0.0, 1.0, C.byref(out)) == L.LDW_ERR_ARG
    for other in (L.PLOT_SR_CLUST, L.PLOT_LDMAP, 6, -1):
        assert lib.ldw_plot_xy_layout_get(other, 1, 0.0, 1.0, 0.0, 1.0, C.byref(out)) == L.LDW_ERR_ARG


def test_painter_agrees_with_plot_ref_where_the_rules_coincide():
    """One class, no line, the rows drawn in row order with the LATER row on top: plot_ref's fixed-colour painter draws its rows in reverse
    (first row on top) when ordered, so it is given the rows reversed."""
    rng = np.random.default_rng(5)
    n, W, H = 400, 97, 70
    x, y = np.floor(rng.random(n) * 300.0), rng.random(n) ** 2
    x[7], y[9] = np.nan, np.inf
    xr, yr = R.data_ranges(x, y)
    assert (xr, yr) == X.data_ranges(x, y)
    _, _, xt = P.ticks(xr[0], xr[1], W, False)
    _, _, yt = P.ticks(yr[0], yr[1], H, True)
    for D in (1, 5, 11):
        got, dropped = X.paint(x, y, None, 1, [0x123456], W, H, D, xt, yt)
        want = R.naive_painter(x[::-1], y[::-1], None, None, None, 1, W, H, D, True, xt, yt, layer_rgb=(0, 0x123456))[0]
        assert dropped == 2 and np.array_equal(got, want), D


def test_painter_on_a_hand_made_case():
    """Three points on a 9 x 7 panel, D = 3; the later row wins; a horizontal line of width 1 through the middle covers both."""
    x, y, cls = np.array([0.0, 4.0, 5.0, 8.0]), np.array([0.0, 3.0, 3.0, 6.0]), np.array([0, 1, 2, 0])
    col = [0x000001, 0x000002, 0x000003]
    img, _ = X.paint(x, y, cls, 3, col, 9, 7, 3, [], [])
    sym = {R.BG: ".", (0, 0, 1): "a", (0, 0, 2): "b", (0, 0, 3): "c", (255, 0, 0): "L"}
    rows = ["".join(sym[tuple(p)] for p in row) for row in img]
    assert rows == [".......aa", ".......aa", "...bccc..", "...bccc..", "...bccc..", "aa.......", "aa......."], rows
    img, _ = X.paint(x[[0, 2, 1, 3]], y[[0, 2, 1, 3]], cls[[0, 2, 1, 3]], 3, col, 9, 7, 3, [], [])
    assert ["".join(sym[tuple(p)] for p in row) for row in img][2:5] == ["...bbbc..", "...bbbc..", "...bbbc.."]
    img, _ = X.paint(x, y, cls, 3, col, 9, 7, 3, [], [], lx=[0.0, 8.0], ly=[3.0, 3.0], line_w=1)
    assert ["".join(sym[tuple(p)] for p in row) for row in img][2:5] == ["...bccc..", "LLLLLLLLL", "...bccc.."]
    with pytest.raises(ValueError):
        X.paint(x, y, cls, 2, col, 9, 7, 3, [], [])
    # a NaN vertex breaks the path: one segment, nothing, one isolated vertex (a disc of diameter line_w)
    segs = X.segments(np.array([0.0, 4.0, np.nan, 8.0]), np.array([0.0, 3.0, 1.0, 6.0]), -0.4, 8.4, -0.3, 6.3, 9, 7)
    assert segs == [(0, 6, 4, 3), (8, 0, 8, 0)]


def test_cabi_refusals_without_a_device():
    lib = L.lib()
    x = np.zeros(4)
    rgb = np.zeros((4, 4, 3), dtype=np.uint8)
    o = P.xy_opts(L.PLOT_FIT)
    assert lib.ldw_plot_xy(None, L.ptr(x), L.ptr(x), None, 4, 0, None, None, 0, C.byref(o), None, None, None, b"x.png", None, None) == L.LDW_ERR_ARG
    assert "null context" in lib.ldw_last_error().decode()
    assert lib.ldw_debug_plot_xy_panel(None, L.ptr(x), L.ptr(x), None, 4, 0, None, None, 0, C.byref(o), 4, 4, L.ptr(rgb), None, None) == L.LDW_ERR_ARG
    import ldweaver_amd
    assert "LDWeaver" in ldweaver_amd.__all__ and "cleanup" in ldweaver_amd.__all__
