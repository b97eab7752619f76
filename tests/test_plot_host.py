"""The host side of the plots (include/ldweaver_amd.h 12): PNG writer, figure layout, ticks, colour tables, the two tsv
readers, make_gwes_plots' argument checks and the C ABI's refusals that need no device.  Runs without a GPU."""
import ctypes as C
import itertools
import os
import zlib

import numpy as np
import pandas as pd
import pytest

import plot_ref as R
from ldweaver_amd import _lib as L
from ldweaver_amd import plots as P


@pytest.mark.parametrize("w,h", [(1, 1), (3, 5), (17, 1), (1, 19), (255, 33), (4800, 1200)])
def test_png_round_trip(tmp_path, w, h):
    rng = np.random.default_rng(w * 7919 + h)
    rgb = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    path = tmp_path / "a.png"
    nbytes = P.png_write(path, rgb)
    data = path.read_bytes()
    assert nbytes == len(data)
    got, ihdr = R.png_decode(data)          # (checks the signature, every chunk's CRC and the IHDR fields 8 / 2 / 0 / 0 / 0)
    assert ihdr[:2] == (w, h)
    assert np.array_equal(got, rgb)


def test_png_levels_and_flat_canvas(tmp_path):
    flat = np.full((300, 400, 3), 255, dtype=np.uint8)
    sizes = []
    for lv in (0, 1, 9):
        n = P.png_write(tmp_path / f"l{lv}.png", flat, level=lv)
        assert np.array_equal(R.png_decode((tmp_path / f"l{lv}.png").read_bytes())[0], flat)
        sizes.append(n)
    assert sizes[0] > 300 * 400 * 3 and sizes[2] < 4000


def test_png_decoder_reads_all_filter_types():
    """The test suite's own decoder: a hand-filtered image with one row of every filter type."""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(5, 4, 3), dtype=np.int64)
    flat = img.reshape(5, 12)
    rows = []
    for j, f in enumerate((0, 1, 2, 3, 4)):
        up = flat[j - 1] if j else np.zeros(12, dtype=np.int64)
        enc = []
        for i in range(12):
            a = flat[j, i - 3] if i >= 3 else 0
            b, c = up[i], (up[i - 3] if i >= 3 else 0)
            p = a + b - c
            paeth = a if (abs(p - a) <= abs(p - b) and abs(p - a) <= abs(p - c)) else (b if abs(p - b) <= abs(p - c) else c)
            pred = (0, a, b, (a + b) // 2, paeth)[f]
            enc.append((flat[j, i] - pred) & 255)
        rows.append(bytes([f] + enc))

    def chunk(t, body):
        return len(body).to_bytes(4, "big") + t + body + (zlib.crc32(t + body) & 0xFFFFFFFF).to_bytes(4, "big")
    data = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", (4).to_bytes(4, "big") + (5).to_bytes(4, "big") + bytes([8, 2, 0, 0, 0]))
            + chunk(b"IDAT", zlib.compress(b"".join(rows))) + chunk(b"IEND", b""))
    assert np.array_equal(R.png_decode(data)[0], img.astype(np.uint8))


def _disjoint(a, b):
    return a[0] + a[2] <= b[0] or b[0] + b[2] <= a[0] or a[1] + a[3] <= b[1] or b[1] + b[3] <= a[1]


def _is_125_multiple(ticks):
    """Every tick is an integer multiple of one step m * 10^e, m in {1, 2, 5}."""
    ticks = np.asarray(ticks, dtype=np.float64)
    if len(ticks) < 2:
        return len(ticks) == 1
    step = np.diff(ticks).min()
    # a difference of two ticks carries their rounding errors: relative to the step that is eps * |tick| / step
    rel = 1e-9 + 8 * np.finfo(np.float64).eps * np.abs(ticks).max() / step
    e = np.floor(np.log10(step) + 1e-6)
    m = step / 10.0 ** e
    near = min((1, 2, 5, 10), key=lambda k: abs(m - k))
    if abs(m - near) > 10 * rel:
        return False
    q = ticks / (near * 10.0 ** e)      # against the exact 1-2-5 step
    return bool(np.all(np.abs(q - np.round(q)) <= rel * np.maximum(np.abs(q), 1.0)))


@pytest.mark.parametrize("n", range(1, 11))
def test_layout_facet_grids(n):
    grid = {1: (1, 1), 2: (1, 2), 3: (1, 3), 4: (2, 2), 5: (2, 3), 6: (2, 3), 7: (3, 3), 8: (3, 3), 9: (3, 3), 10: (3, 4)}[n]
    lay = P.layout(L.PLOT_SR_CLUST, n, (13.0, 49871.0), (0.0123, 0.73))
    assert (lay["rows"], lay["cols"]) == grid and (lay["width"], lay["height"]) == (2200, 1200)
    assert len(lay["panels"]) == n and len(lay["strips"]) == n and lay["cbar"] is not None
    rects = lay["panels"] + lay["strips"] + [lay["cbar"]]
    for r in rects:
        assert r[0] >= 0 and r[1] >= 0 and r[2] > 0 and r[3] > 0 and r[0] + r[2] <= 2200 and r[1] + r[3] <= 1200, r
    for a, b in itertools.combinations(rects, 2):
        assert _disjoint(a, b), (a, b)
    assert all(p[2] == lay["panel_w"] and p[3] == lay["panel_h"] for p in lay["panels"])
    for k, p in enumerate(lay["panels"]):                       # row-major facets
        assert p[0] == lay["panels"][k % grid[1]][0] and p[1] == lay["panels"][(k // grid[1]) * grid[1]][1]


@pytest.mark.parametrize("kind,size,cbar", [(L.PLOT_SR_COMBI, (2200, 1200), True), (L.PLOT_LR, (4800, 1200), False), (L.PLOT_LDMAP, (5000, 5250), False)])
def test_layout_single_panel_figures(kind, size, cbar):
    lay = P.layout(kind, 1, (20000.0, 2.1e6), (0.05, 0.4))
    assert (lay["width"], lay["height"]) == size and (lay["rows"], lay["cols"]) == (1, 1) and not lay["strips"]
    assert (lay["cbar"] is not None) == cbar
    x, y, w, h = lay["panels"][0]
    assert x > 0 and y > 0 and x + w < size[0] and y + h < size[1]
    if kind == L.PLOT_LDMAP:
        assert w == h and not lay["xticks"] and not lay["yticks"]
    with pytest.raises(L.LdwError):
        P.layout(kind, 2)


@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (13.0, 49871.0), (0.0123, 0.73), (-3.5e-7, 2.2e-7), (5.0, 5.0), (0.0, 0.0), (1e9, 3.7e9), (-120.0, -3.0),
                                   (0.1, 0.1000001), (2.0, 1.4e6)])
def test_ticks(lo, hi):
    for npx, flip in ((640, False), (330, True), (1, False), (4570, False)):
        lim, t, px = P.ticks(lo, hi, npx, flip)
        want = R.axis_range(lo, hi)
        assert lim == (float(want[0]), float(want[1]))
        assert 3 <= len(t) <= 10 and np.all(np.diff(t) > 0)
        assert t[0] >= lim[0] and t[-1] <= lim[1]
        assert _is_125_multiple(t), t
        want_px = R.pixel(t, lim[0], lim[1], npx)
        assert np.array_equal(px, npx - 1 - want_px if flip else want_px)
    lay = P.layout(L.PLOT_SR_CLUST, 4, (lo, hi), (lo, hi))
    assert lay["xlim"] == lay["ylim"] == (float(want[0]), float(want[1]))
    assert np.array_equal(lay["xtick_px"], R.pixel(lay["xticks"], *lay["xlim"], lay["panel_w"]))
    assert np.array_equal(lay["ytick_px"], lay["panel_h"] - 1 - R.pixel(lay["yticks"], *lay["ylim"], lay["panel_h"]))


def test_colour_tables_equal_the_numpy_rules():
    assert np.array_equal(P.ramp_colours(), R.ramp())
    ramp = R.ramp()
    assert tuple(ramp[0]) == (255, 255, 255) and tuple(ramp[685]) == (0xE1, 0xB9, 0xB4) and tuple(ramp[1370]) == (0xAE, 0x45, 0x2C)
    assert tuple(ramp[2055]) == (0x80, 0x24, 0x18)
    rng = np.random.default_rng(11)
    t = np.concatenate([rng.random(200_000), np.arange(6) / 5.0, [0.5, np.nextafter(1.0, 0), np.nextafter(0.2, 0), np.nextafter(0.2, 1)]])
    assert np.array_equal(P.gradient_colours(t), R.gradient(t))
    assert [tuple(c) for c in R.gradient(np.arange(6) / 5.0)] == [tuple(int(v) for v in s) for s in R.STOPS]


def test_reference_painter_on_a_hand_made_case():
    """Five points on a 9 x 7 panel, D = 3 (a 3 x 3 square): A grey under everything; B and C direct with srp 1 < 2 overlapping (C on top);
    D direct with C's srp in B's pixel (ties B out); E dropped (NaN).  Axis range of [0, 8] x [0, 6] widened by 5 %."""
    x = np.array([1.0, 4.0, 5.0, 4.0, np.nan, 0.0, 8.0])
    y = np.array([1.0, 3.0, 3.0, 3.0, 2.0, 0.0, 6.0])
    srp = np.array([9.0, 1.0, 2.0, 2.0, 5.0, 1.0, 1.0])
    layer = np.array([0, 1, 1, 1, 1, 0, 0])
    img = R.naive_painter(x, y, srp, layer, None, 1, 9, 7, 3, False, [], [])[0]
    lo, hi = tuple(R.gradient([0.0])[0]), tuple(R.gradient([1.0])[0])
    assert lo == (0x45, 0x75, 0xB4) and hi == (0xD7, 0x30, 0x27)
    sym = {R.BG: ".", R.GREY: "g", lo: "b", hi: "r"}
    rows = ["".join(sym[tuple(p)] for p in row) for row in img]
    # pixel rule: x0 = -0.4, x1 = 8.4, W = 9: px = floor((x + 0.4) / 8.8 * 9) -> 1, 4, 5, 4, -, 0, 8; y likewise -> py = 6 - (1, 3, 3, 3, -, 0, 6)
    assert rows == [".......gg",
                    ".......gg",
                    "...rrrr..",
                    "...rrrr..",
                    "gggrrrr..",
                    "ggg......",
                    "ggg......"], rows
    # row order as the draw order (first row on top): the rows are drawn in reverse, so B (row 1) comes after C (row 2) and D (row 3) and
    # covers both inside its own square
    img = R.naive_painter(x, y, srp, layer, None, 1, 9, 7, 3, True, [], [])[0]
    rows = ["".join(sym[tuple(p)] for p in row) for row in img]
    assert rows[2:5] == ["...bbbr..", "...bbbr..", "gggbbbr.."], rows


def test_readers(tmp_path):
    sr = tmp_path / "sr.tsv"
    sr.write_text("1\t100\t2300\t1\t1\t2200\t0.31\t4.5\t1\n2\t500\t900\t2\t3\t400\t0.2\t3.25\t0\n")
    df = P.read_ShortRangeLinks(sr)
    assert list(df.columns) == P.SR_COLS and df.shape == (2, 9) and df["srp_max"].tolist() == [4.5, 3.25] and df["ARACNE"].tolist() == [1, 0]
    lr = tmp_path / "lr.tsv"
    lr.write_text("100\t50000\t1\t2\t49900\t0.11\n200\t9000\t1\t1\t8800\t0.5\n300\t90000\t2\t2\t89700\t0.07\n")
    df = P.read_LongRangeLinks(lr)
    assert list(df.columns) == P.LR_COLS and df["len"].tolist() == [49900, 89700]          # len < sr_dist dropped
    assert P.read_LongRangeLinks(lr, sr_dist=100)["len"].tolist() == [49900, 8800, 89700]
    sp5 = tmp_path / "sp5.txt"
    sp5.write_text("100 50000 49900 1 0.11\n200 9000 8800 0 0.5\n")
    df = P.read_LongRangeLinks(sp5, links_from_spydrpick=True)
    assert list(df.columns) == ["pos1", "pos2", "len", "ARACNE", "MI"] and df["MI"].tolist() == [0.11]
    sp4 = tmp_path / "sp4.txt"
    sp4.write_text("100 50000 49900 0.11\n200 90000 89800 0.5\n")
    df = P.read_LongRangeLinks(sp4, links_from_spydrpick=True)
    assert list(df.columns) == ["pos1", "pos2", "len", "MI"] and len(df) == 2
    import ldweaver_amd
    assert ldweaver_amd.read_ShortRangeLinks is P.read_ShortRangeLinks and ldweaver_amd.make_gwes_plots is P.make_gwes_plots


def test_make_gwes_plots_argument_errors(tmp_path):
    folder = str(tmp_path / "PL")
    six = pd.DataFrame(np.zeros((2, 6)))
    nine = pd.DataFrame(np.zeros((2, 9)))
    with pytest.raises(ValueError) as e:
        P.make_gwes_plots(sr_links=six, plt_folder=folder)
    assert str(e.value) == "sr_links must either be (1) a data.frame with sr_links or (2) the path to the saved tsv file from perform_MI_computation()"
    with pytest.raises(ValueError) as e:
        P.make_gwes_plots(lr_links=nine, plt_folder=folder)
    assert str(e.value) == "lr_links must either be (1) a data.frame with lr_links or (2) the path to the saved tsv file from perform_MI_computation()"
    with pytest.raises(ValueError, match="^sr_links must either be"):
        P.make_gwes_plots(sr_links=str(tmp_path / "nothing_here.tsv"), plt_folder=folder)
    with pytest.raises(ValueError, match="^lr_links must either be"):
        P.make_gwes_plots(lr_links=str(tmp_path / "nothing_here.tsv"), plt_folder=folder)
    assert P.make_gwes_plots(plt_folder=folder) == {} and os.path.isdir(folder)      # nothing to draw: the folder is still made
    many = pd.DataFrame(np.zeros((11, 9)), columns=P.SR_COLS)
    many["clust_c"] = np.arange(11)
    with pytest.raises(ValueError, match="at most 10"):
        P.sr_facets(many["clust_c"])
    panel, labels = P.sr_facets(np.array([7, 2, 2, 9, 7]))
    assert panel.tolist() == [1, 0, 0, 2, 1] and labels.tolist() == [2, 7, 9]


def test_cabi_refusals_without_a_device(tmp_path):
    lib = L.lib()
    msg = lambda: lib.ldw_last_error().decode()
    rgb = np.zeros((2, 2, 3), dtype=np.uint8)
    x = np.zeros(4)
    o = P.plot_opts(L.PLOT_SR_COMBI)
    n64 = C.c_int64(0)
    assert lib.ldw_plot_scatter(None, L.ptr(x), L.ptr(x), None, None, None, 4, 0, C.byref(o), 1, None, b"x.png", None, None) == L.LDW_ERR_ARG
    assert "null context" in msg()
    assert lib.ldw_plot_links(None, 0, 1, C.byref(o), b"x.png", None, None) == L.LDW_ERR_ARG and "null context" in msg()
    assert lib.ldw_plot_heatmap(None, L.ptr(x), 2, 0, None, b"x.png", None) == L.LDW_ERR_ARG and "null context" in msg()
    n_pos, r, B = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    assert lib.ldw_plot_ldmap(None, 0, 0, 0, None, b"x.png", C.byref(n_pos), C.byref(r), C.byref(B), None, 0) == L.LDW_ERR_ARG
    assert lib.ldw_debug_plot_panels(None, L.ptr(x), L.ptr(x), None, None, None, 4, 0, C.byref(o), 1, 8, 8, L.ptr(rgb), None, None, None) == L.LDW_ERR_ARG
    # the PNG writer
    assert lib.ldw_png_write(None, L.ptr(rgb), 2, 2, -1, None) == L.LDW_ERR_ARG
    assert lib.ldw_png_write(b"x.png", None, 2, 2, -1, None) == L.LDW_ERR_ARG
    assert lib.ldw_png_write(os.fsencode(tmp_path / "z.png"), L.ptr(rgb), 0, 2, -1, None) == L.LDW_ERR_ARG
    assert lib.ldw_png_write(os.fsencode(tmp_path / "z.png"), L.ptr(rgb), 2, 2, 10, None) == L.LDW_ERR_ARG
    bad = os.fsencode(tmp_path / "no_such_folder" / "z.png")
    assert lib.ldw_png_write(bad, L.ptr(rgb), 2, 2, -1, C.byref(n64)) == L.LDW_ERR_ARG and "no_such_folder" in msg()
    assert not os.path.exists(tmp_path / "z.png")
    # layout and ticks
    lay = L.PlotLayout()
    assert lib.ldw_plot_layout_get(L.PLOT_SR_CLUST, 3, 0.0, 1.0, 0.0, 1.0, None) == L.LDW_ERR_ARG
    for kind, n in ((-1, 1), (4, 1), (L.PLOT_SR_CLUST, 0), (L.PLOT_SR_CLUST, 11), (L.PLOT_LR, 2)):
        assert lib.ldw_plot_layout_get(kind, n, 0.0, 1.0, 0.0, 1.0, C.byref(lay)) == L.LDW_ERR_ARG, (kind, n)
    assert lib.ldw_plot_layout_get(L.PLOT_LR, 1, 0.0, float("nan"), 0.0, 1.0, C.byref(lay)) == L.LDW_ERR_ARG
    assert lib.ldw_plot_layout_get(L.PLOT_LR, 1, 2.0, 1.0, 0.0, 1.0, C.byref(lay)) == L.LDW_ERR_ARG
    lim, t, px, n = np.zeros(2), np.zeros(16), np.zeros(16, dtype=np.int32), C.c_int32(0)
    assert lib.ldw_plot_ticks(0.0, float("inf"), 100, 0, L.ptr(lim), L.ptr(t), L.ptr(px), C.byref(n)) == L.LDW_ERR_ARG
    assert lib.ldw_plot_ticks(-1.7e308, 1.7e308, 100, 0, L.ptr(lim), L.ptr(t), L.ptr(px), C.byref(n)) == L.LDW_ERR_ARG      # the widened range overflows
    assert lib.ldw_plot_layout_get(L.PLOT_LR, 1, 0.0, 1.0, -1.7e308, 1.7e308, C.byref(lay)) == L.LDW_ERR_ARG
    assert lib.ldw_plot_ticks(0.0, 1.0, 0, 0, L.ptr(lim), L.ptr(t), L.ptr(px), C.byref(n)) == L.LDW_ERR_ARG
    assert lib.ldw_plot_ticks(0.0, 1.0, 100, 0, None, L.ptr(t), L.ptr(px), C.byref(n)) == L.LDW_ERR_ARG
    assert lib.ldw_debug_plot_colours(2, None, 0, L.ptr(rgb)) == L.LDW_ERR_ARG
