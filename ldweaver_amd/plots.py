"""The plots of the reference rendered on the device and written as PNG (include/ldweaver_amd.h 12):
``make_gwes_plots`` (R/prepareGWESplots.R:25-126), the readers it uses (R/io_functions.R:32-66), and the helpers behind the
``lr_gwes.png`` of ``analyse_long_range_links`` (R/lr_analyser.R:117-127) and the ``LD_plot.png`` of ``genomewide_LDMap``
(R/LDSummaryPlot.R:121-128).  The points are reduced to pixels by HIP kernels (one atomic maximum per row, no sort); the frame
round the panels (ticks, labels, strips, colour bar) and the PNG file are written by the library's host code."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L

SR_COLS = ["clust_c", "pos1", "pos2", "clust1", "clust2", "len", "MI", "srp_max", "ARACNE"]   # R/io_functions.R:63
LR_COLS = ["pos1", "pos2", "c1", "c2", "len", "MI"]                                            # R/io_functions.R:35
# every colour the frame uses outside the panels, the strips and the colour bar: background, lines / strips, tick labels, titles
FRAME_COLOURS = ((0xFF, 0xFF, 0xFF), (0xB3, 0xB3, 0xB3), (0x4D, 0x4D, 0x4D), (0x00, 0x00, 0x00))
GREY, LR_DIRECT, LR_LINE = 0xC0C0C0, 0x0868AC, 0xDB4325     # R/lr_analyser.R:120-122
CANVAS = {L.PLOT_SR_CLUST: (2200, 1200), L.PLOT_SR_COMBI: (2200, 1200), L.PLOT_LR: (4800, 1200), L.PLOT_LDMAP: (5000, 5250),
          L.PLOT_FIT: (2200, 1200), L.PLOT_CDS: (2200, 1200)}
FIT_LINE = 0xFF0000                                           # R/computePairwiseMI.R:434
FIT_LABELS = ("Basepair separation", "MI (95th percentile)")  # R/computePairwiseMI.R:435-436
CDS_LABELS = ("Genomic starting position of CDS", "Diversity within CDS")   # R/estimateCDSDiversity.R:216-217
SR_ERR = "sr_links must either be (1) a data.frame with sr_links or (2) the path to the saved tsv file from perform_MI_computation()"
LR_ERR = "lr_links must either be (1) a data.frame with lr_links or (2) the path to the saved tsv file from perform_MI_computation()"


def layout(kind: int, n_panels: int = 1, xr=(0.0, 1.0), yr=(0.0, 1.0)) -> dict:
    """The figure of ``kind`` (``_lib.PLOT_*``) with ``n_panels`` facets for the DATA ranges xr, yr: canvas size, facet grid, panel /
    strip / colour-bar rectangles (x, y, w, h; top-left origin), axis ranges and ticks in data and panel-pixel coordinates.  Host only."""
    lay = L.PlotLayout()
    get = L.lib().ldw_plot_xy_layout_get if int(kind) in (L.PLOT_FIT, L.PLOT_CDS) else L.lib().ldw_plot_layout_get
    L.check(get(int(kind), int(n_panels), float(xr[0]), float(xr[1]), float(yr[0]), float(yr[1]), C.byref(lay)))
    n = lay.n_panels
    return dict(width=lay.width, height=lay.height, n_panels=n, rows=lay.rows, cols=lay.cols, panel_w=lay.panel_w, panel_h=lay.panel_h,
                panels=[tuple(lay.panel[p]) for p in range(n)], strips=[tuple(lay.strip[p]) for p in range(n) if lay.strip[p][2] > 0],
                cbar=tuple(lay.cbar) if lay.cbar[2] > 0 else None, xlim=tuple(lay.xlim), ylim=tuple(lay.ylim),
                xticks=list(lay.xtick[:lay.n_xticks]), yticks=list(lay.ytick[:lay.n_yticks]),
                xtick_px=list(lay.xtick_px[:lay.n_xticks]), ytick_px=list(lay.ytick_px[:lay.n_yticks]))


def ticks(lo: float, hi: float, npx: int, flip: bool = False):
    """Axis range, 1-2-5 tick positions and their pixel offsets for the data range [lo, hi] on an axis of ``npx`` pixels.  Host only."""
    lim, t, px, n = np.zeros(2), np.zeros(L.PLOT_MAX_TICKS), np.zeros(L.PLOT_MAX_TICKS, dtype=np.int32), C.c_int32(0)
    L.check(L.lib().ldw_plot_ticks(float(lo), float(hi), int(npx), int(flip), L.ptr(lim), L.ptr(t), L.ptr(px), C.byref(n)))
    return (float(lim[0]), float(lim[1])), t[:n.value].copy(), px[:n.value].copy()


def png_write(path, rgb, level: int = -1) -> int:
    """8-bit RGB, non-interlaced PNG of ``rgb`` (height, width, 3) uint8.  Returns the bytes written.  Host only."""
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("png_write wants an array of shape (height, width, 3)")
    n = C.c_int64(0)
    L.check(L.lib().ldw_png_write(os.fsencode(path), L.ptr(rgb), rgb.shape[1], rgb.shape[0], int(level), C.byref(n)))
    return n.value


def ramp_colours() -> np.ndarray:
    """The LD map's 2056 colours, (2056, 3) uint8."""
    out = np.zeros((2056, 3), dtype=np.uint8)
    L.check(L.lib().ldw_debug_plot_colours(0, None, 0, L.ptr(out)))
    return out


def gradient_colours(t) -> np.ndarray:
    """The scatter gradient at t in [0, 1], (n, 3) uint8."""
    t = np.ascontiguousarray(t, dtype=np.float64)
    out = np.zeros((len(t), 3), dtype=np.uint8)
    L.check(L.lib().ldw_debug_plot_colours(1, L.ptr(t), len(t), L.ptr(out)))
    return out


def plot_opts(kind: int, D: int = 11, ordered: bool = False, layer_rgb=(GREY, 0), hline=None, hline_rgb: int = LR_LINE,
              no_precheck: bool = False) -> L.PlotOpts:
    o = L.PlotOpts()
    o.kind, o.D, o.ordered, o.flags = int(kind), int(D), int(bool(ordered)), L.PLOT_NO_PRECHECK if no_precheck else 0
    o.layer_rgb[0], o.layer_rgb[1] = int(layer_rgb[0]), int(layer_rgb[1])
    o.has_hline, o.hline_y, o.hline_rgb = (0, 0.0, 0) if hline is None else (1, float(hline), int(hline_rgb))
    return o


SCATTER_COLS = (("x", "float64"), ("y", "float64"), ("srp", "float64"), ("layer", "uint8"), ("panel", "uint8"))
XY_COLS = (("x", "float64"), ("y", "float64"), ("cls", "uint8"))


def _columns(spec, *arrays):
    """The columns ``arrays`` (None: not given) of the (name, dtype) list ``spec`` as C-contiguous arrays of the C ABI's types: numpy (host) or
    torch tensors on the GPU (device), as the first one is.  Returns (columns, rows, on the device)."""
    dev = hasattr(arrays[0], "data_ptr") and bool(getattr(arrays[0], "is_cuda", False))
    cols = []
    for a, (_, dt) in zip(arrays, spec):
        if a is None:
            cols.append(None)
        elif dev:
            import torch
            cols.append(a.to(getattr(torch, dt)).contiguous())
        else:
            cols.append(np.ascontiguousarray(a, dtype=dt))
    if dev:
        import torch
        torch.cuda.current_stream().synchronize()   # the library reads the columns on the engine's stream: what torch has queued must be done
    n = len(cols[0])
    if any(c is not None and len(c) != n for c in cols):
        raise ValueError("the columns differ in length")
    return cols, n, dev


def render_scatter(eng, x, y, srp=None, layer=None, panel=None, *, opts: L.PlotOpts, n_panels: int = 1, labels=None, path=None,
                   want_canvas: bool = False):
    """One scatter figure (ldw_plot_scatter).  Returns (canvas or None, rows dropped)."""
    cols, n, dev = _columns(SCATTER_COLS, x, y, srp, layer, panel)
    W, H = CANVAS[opts.kind]
    canvas = np.zeros((H, W, 3), dtype=np.uint8) if want_canvas else None
    lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.int32)
    dropped = C.c_int64(0)
    L.check(L.lib().ldw_plot_scatter(eng._ctx, *[L.ptr(c) for c in cols], n, int(dev), C.byref(opts), int(n_panels), L.ptr(lab),
                                     None if path is None else os.fsencode(path), L.ptr(canvas), C.byref(dropped)))
    return canvas, dropped.value


def render_links(eng, which: int, *, opts: L.PlotOpts, use_aracne: bool = True, path=None, want_canvas: bool = False):
    """The same from the engine's resident kept links (ldw_plot_links): nothing is copied to the host.  ``use_aracne``: the layers are the
    flags ``ldw_aracne_device`` left for these links (the library refuses if it has not run for them); False: every link is drawn as direct."""
    if not hasattr(eng, "_ctx"):
        raise TypeError(f"the resident links are those of one Engine; got {type(eng).__name__} (for several engines pass the one that holds the "
                        "kept links, engines[0])")
    W, H = CANVAS[opts.kind]
    canvas = np.zeros((H, W, 3), dtype=np.uint8) if want_canvas else None
    dropped = C.c_int64(0)
    L.check(L.lib().ldw_plot_links(eng._ctx, int(which), int(bool(use_aracne)), C.byref(opts), None if path is None else os.fsencode(path),
                                   L.ptr(canvas), C.byref(dropped)))
    return canvas, dropped.value


def debug_panels(eng, x, y, srp=None, layer=None, panel=None, *, opts: L.PlotOpts, n_panels: int = 1, W: int, H: int, timing: bool = False):
    """The rasters without the frame (ldw_debug_plot_panels): (rgb (n_panels, H, W, 3), stats dict, scratch bytes, ms or None)."""
    cols, n, dev = _columns(SCATTER_COLS, x, y, srp, layer, panel)
    out = np.zeros((n_panels, H, W, 3), dtype=np.uint8)
    st, ms, scratch = np.zeros(8), np.zeros(4), C.c_int64(0)
    L.check(L.lib().ldw_debug_plot_panels(eng._ctx, *[L.ptr(c) for c in cols], n, int(dev), C.byref(opts), int(n_panels), int(W), int(H),
                                          L.ptr(out), L.ptr(st), C.byref(scratch), L.ptr(ms) if timing else None))
    stats = dict(xr=(st[0], st[1]), yr=(st[2], st[3]), lo=st[4], hi=st[5], kept=int(st[6]), dropped=int(st[7]))
    return out, stats, scratch.value, (dict(stats=ms[0], clear=ms[1], centre=ms[2], disc=ms[3]) if timing else None)


def xy_opts(kind: int, D: int = 11, class_rgb=(0,), line_w: int = 5, line_rgb: int = FIT_LINE) -> L.PlotXYOpts:
    o = L.PlotXYOpts()
    o.kind, o.D, o.n_classes, o.line_w, o.line_rgb = int(kind), int(D), len(class_rgb), int(line_w), int(line_rgb)
    for k, v in enumerate(class_rgb[:L.PLOT_MAX_CLASSES]):
        o.class_rgb[k] = int(v)
    return o


def _xy_columns(x, y, cls, line):
    """x, y, cls through ``_columns`` and the line's vertices as host arrays."""
    cols, n, dev = _columns(XY_COLS, x, y, cls)
    lx, ly = (None, None) if line is None else (np.ascontiguousarray(line[0], dtype=np.float64), np.ascontiguousarray(line[1], dtype=np.float64))
    if lx is not None and len(lx) != len(ly):
        raise ValueError("the line's vertex arrays differ in length")
    return cols, n, dev, lx, ly


def _text(s):
    return None if s is None else str(s).encode()


def render_xy(eng, x, y, cls=None, line=None, *, opts: L.PlotXYOpts, title=None, xlab=None, ylab=None, path=None, want_canvas: bool = False):
    """One xy figure (ldw_plot_xy): points in row order, the later row on top, coloured by class; ``line`` = (x, y) vertices of a polyline drawn
    over them.  Returns (canvas or None, rows dropped)."""
    cols, n, dev, lx, ly = _xy_columns(x, y, cls, line)
    W, H = CANVAS[opts.kind]
    canvas = np.zeros((H, W, 3), dtype=np.uint8) if want_canvas else None
    dropped = C.c_int64(0)
    L.check(L.lib().ldw_plot_xy(eng._ctx, *[L.ptr(c) for c in cols], n, int(dev), L.ptr(lx), L.ptr(ly), 0 if lx is None else len(lx), C.byref(opts),
                                _text(title), _text(xlab), _text(ylab), None if path is None else os.fsencode(path), L.ptr(canvas), C.byref(dropped)))
    return canvas, dropped.value


def debug_xy_panel(eng, x, y, cls=None, line=None, *, opts: L.PlotXYOpts, W: int, H: int, timing: bool = False):
    """The panel without the frame (ldw_debug_plot_xy_panel): (rgb (H, W, 3), stats dict, ms or None)."""
    cols, n, dev, lx, ly = _xy_columns(x, y, cls, line)
    out = np.zeros((H, W, 3), dtype=np.uint8)
    st, ms = np.zeros(6), np.zeros(4)
    L.check(L.lib().ldw_debug_plot_xy_panel(eng._ctx, *[L.ptr(c) for c in cols], n, int(dev), L.ptr(lx), L.ptr(ly), 0 if lx is None else len(lx),
                                            C.byref(opts), int(W), int(H), L.ptr(out), L.ptr(st), L.ptr(ms) if timing else None))
    stats = dict(xr=(st[0], st[1]), yr=(st[2], st[3]), kept=int(st[4]), dropped=int(st[5]))
    return out, stats, (dict(stats=ms[0], clear=ms[1], centre=ms[2], paint=ms[3]) if timing else None)


def _with_engine(engine, fn):
    from .engine import Engine
    own = engine is None
    eng = Engine(0) if own else engine
    try:
        return fn(eng)
    finally:
        if own:
            eng.close()


def fit_plot(fit_data_i, i: int, path, *, engine=None) -> str:
    """``c<i>_fit.png`` (R/computePairwiseMI.R:430-440): the per-distance 95th percentile ``max`` against ``len`` as black points, the fitted
    curve (``len``, ``fit``) as a red line over them, titled ``Clust i``.  ``fit_data_i``: a frame with the columns len, max, fit, ascending in
    len (what ``perform_MI_computation`` writes to ``c<i>_fit_data.tsv``).  Returns the path."""
    ln = np.asarray(fit_data_i["len"], dtype=np.float64)
    mx = np.asarray(fit_data_i["max"], dtype=np.float64)
    ft = np.asarray(fit_data_i["fit"], dtype=np.float64)
    _with_engine(engine, lambda eng: render_xy(eng, ln, mx, None, (ln, ft), opts=xy_opts(L.PLOT_FIT), title=f"Clust {int(i)}", xlab=FIT_LABELS[0],
                                               ylab=FIT_LABELS[1], path=path))
    return str(path)


DECAY_LABELS = ("Basepair separation (upper edge of the bin)", "MI quantile")


def ld_decay_plot(decay, path, q: float = 0.95, *, engine=None) -> str:
    """The LD-decay curve of ``decay`` (``decay.LDDecay``): the q-quantile of the MI (its lo) of every distance bin that holds a pair against the bin's
    upper edge as black points, and the background level (``decay.background(q)``; left out when no bin lies at or beyond g / 4) as a red line across,
    in the layout of the fit figures (PLOT_FIT).  Returns the path."""
    qlo, _ = decay.quantile(q)
    keep = np.isfinite(qlo)
    x, y = np.asarray(decay.len_hi, dtype=np.float64)[keep], qlo[keep]
    try:
        bg = decay.background(q)[0]
        line = (np.array([x.min(), x.max()]), np.array([bg, bg])) if len(x) else None
    except ValueError:
        line = None
    _with_engine(engine, lambda eng: render_xy(eng, x, y, None, line, opts=xy_opts(L.PLOT_FIT), title=f"LD decay (q = {q:g})", xlab=DECAY_LABELS[0],
                                               ylab=DECAY_LABELS[1], path=path))
    return str(path)


BACKGROUND_LABELS = ("Genomic position", "Mean long-range MI")


def snp_background_plot(background, path, *, engine=None) -> str:
    """Of ``background`` (``background.SnpBackground``): the mean long-range MI of every SNP that has a long-range partner against its position as black
    points, and the overall long-range mean as a red line across, in the layout of the fit figures (PLOT_FIT).  Returns the path."""
    y = background.mean("lr")
    keep = np.isfinite(y)
    x, y = np.asarray(background.POS, dtype=np.float64)[keep], y[keep]
    line = (np.array([x.min(), x.max()]), np.full(2, background.overall_mean("lr"))) if len(x) else None
    _with_engine(engine, lambda eng: render_xy(eng, x, y, None, line, opts=xy_opts(L.PLOT_FIT), title="MI background", xlab=BACKGROUND_LABELS[0],
                                               ylab=BACKGROUND_LABELS[1], path=path))
    return str(path)


def cds_cluster_plot(cds_var, path, *, engine=None) -> str:
    """``CDS_clustering.png`` (R/estimateCDSDiversity.R:212-220): ``var_estimate`` against ``cds_start``, coloured by the cluster
    ``km_clst_ord`` in ggplot's default hues, in row order.  Returns the path."""
    from .network import hue_palette
    nclust = int(cds_var.nclust)
    if not 1 <= nclust <= L.PLOT_MAX_CLASSES:
        raise ValueError(f"{nclust} clusters: the figure takes 1..{L.PLOT_MAX_CLASSES}")
    x = np.asarray(cds_var.cds_start, dtype=np.float64)
    y = np.asarray(cds_var.var_estimate, dtype=np.float64)
    cls = (np.asarray(cds_var.clusts["km_clst_ord"]).astype(np.int64) - 1).astype(np.uint8)
    _with_engine(engine, lambda eng: render_xy(eng, x, y, cls, None, opts=xy_opts(L.PLOT_CDS, class_rgb=[int(c) for c in hue_palette(nclust)]),
                                               xlab=CDS_LABELS[0], ylab=CDS_LABELS[1], path=path))
    return str(path)


def render_heatmap(eng, htm, path, title=None):
    """LD_plot.png of a B x B map in [0, 1] (ldw_plot_heatmap)."""
    (h,), _, dev = _columns((("htm", "float64"),), htm)
    if h.ndim != 2 or h.shape[0] != h.shape[1]:
        raise ValueError("the map must be square")
    L.check(L.lib().ldw_plot_heatmap(eng._ctx, L.ptr(h), int(h.shape[0]), int(dev), None if title is None else str(title).encode(),
                                     os.fsencode(path), None))


GENE_MAP_BY = ("frac", "max", "mean")


def gene_map_matrix(gm, by: str = "frac") -> np.ndarray:
    """What ``gene_map_plot`` draws, a pure host function: ``gm.symmetric(by)`` divided by its largest finite value, clipped to [0, 1]; a cell without a
    pair, a non-finite value and everything when no value is positive become 0."""
    if by not in GENE_MAP_BY:
        raise ValueError(f"by must be one of {GENE_MAP_BY}, got {by!r}")
    m = np.asarray(gm.symmetric(by), dtype=np.float64)
    fin = np.isfinite(m)
    top = m[fin].max() if fin.any() else 0.0
    if not top > 0:
        return np.zeros_like(m)
    return np.clip(np.where(fin, m, 0.0) / top, 0.0, 1.0)


def gene_map_plot(gm, path, by: str = "frac", *, engine=None) -> str:
    """Of ``gm`` (``genemap.GeneMap``): the symmetrised segment x segment matrix ``by`` (frac, max or mean), rescaled to [0, 1] by its finite maximum
    (``gene_map_matrix``), as the heat map of ``LD_plot.png`` (ldw_plot_heatmap): segment 0 at the bottom left.  Returns the path."""
    h = gene_map_matrix(gm, by)
    _with_engine(engine, lambda eng: render_heatmap(eng, h, path, title=f"Gene map ({by})"))
    return str(path)


# ---- the readers of R/io_functions.R:32-66 ---------------------------------------------------------------------------------------------------

def read_ShortRangeLinks(sr_links_path, reader: str = "pandas"):
    """sr_links.tsv as a frame with the reference's column names.  ``reader="native"``: parsed on the device (links_io.read_links_native), every value
    the correctly rounded double of its text — pandas' default parser, which ``"pandas"`` keeps, can be one ulp off."""
    from .links_io import check_reader, read_links_native
    if check_reader(reader):
        return read_links_native(sr_links_path, "sr")
    import pandas as pd
    return pd.read_csv(sr_links_path, sep="\t", header=None, names=SR_COLS, quoting=3, comment=None)


def read_LongRangeLinks(lr_links_path, links_from_spydrpick: bool = False, sr_dist=20000, reader: str = "pandas"):
    """lr_links.tsv (tab separated, six columns) or a SpydrPick file (space separated: pos1 pos2 len [ARACNE] MI); links with
    len < sr_dist are dropped.  ``reader``: as in ``read_ShortRangeLinks``."""
    from .links_io import check_reader, read_links_native
    if check_reader(reader):
        return read_links_native(lr_links_path, "spydrpick" if links_from_spydrpick else "lr", sr_dist=sr_dist)
    import pandas as pd
    if not links_from_spydrpick:
        df = pd.read_csv(lr_links_path, sep="\t", header=None, names=LR_COLS, quoting=3, comment=None)
    else:
        df = pd.read_csv(lr_links_path, sep=" ", header=None, quoting=3, comment=None)
        if df.shape[1] == 5:
            df.columns = ["pos1", "pos2", "len", "ARACNE", "MI"]
        elif df.shape[1] == 4:
            df.columns = ["pos1", "pos2", "len", "MI"]
    drops = df["len"] < sr_dist
    if drops.any():
        df = df[~drops].reset_index(drop=True)
    return df


# ---- make_gwes_plots ---------------------------------------------------------------------------------------------------------------------------

def _frame(links, reader, ncol: int, names, err: str):
    import pandas as pd
    if not isinstance(links, pd.DataFrame):
        if not (isinstance(links, (str, bytes)) or hasattr(links, "__fspath__")) or not os.path.exists(links):
            raise ValueError(err)
        links = reader(links)
    if links.shape[1] != ncol:
        raise ValueError(err)
    links = links.copy(deep=False)
    links.columns = names
    return links


def sr_facets(clust_c):
    """Facet of every row: rank of its clust_c among the sorted distinct values (ggplot's facet order).  Returns (panel uint8, labels)."""
    labels, panel = np.unique(np.asarray(clust_c), return_inverse=True)
    if len(labels) > L.PLOT_MAX_PANELS:
        raise ValueError(f"sr_links hold {len(labels)} clusters: the facet figure takes at most {L.PLOT_MAX_PANELS}")
    return panel.astype(np.uint8), labels.astype(np.int32)


def _is_path(links):
    return isinstance(links, (str, bytes)) or hasattr(links, "__fspath__")


def _device_columns(eng, links, kind: str, ncol: int, err: str):
    """The columns of a link file on the engine's GPU (reader="native"): the checks of ``_frame``, no frame."""
    from .links_io import read_links_native, tsv_probe
    if not os.path.exists(links) or tsv_probe(links, "\t")[0] not in (0, ncol):
        raise ValueError(err)
    return read_links_native(links, kind, engine=eng, to="device")


def sr_facets_device(clust_c):
    """``sr_facets`` for a device column: (panel uint8 tensor, labels int32 array)."""
    import torch
    labels, panel = torch.unique(clust_c, sorted=True, return_inverse=True)
    if len(labels) > L.PLOT_MAX_PANELS:
        raise ValueError(f"sr_links hold {len(labels)} clusters: the facet figure takes at most {L.PLOT_MAX_PANELS}")
    return panel.to(torch.uint8), labels.cpu().numpy().astype(np.int32)


def make_gwes_plots(lr_links=None, sr_links=None, plt_folder=None, are_srlinks_ordered: bool = False, *, engine=None, D: int = 11,
                    aracne: bool = True, reader: str = "pandas") -> dict:
    """``make_gwes_plots`` of the reference: ``lr_gwes.png`` from ``lr_links`` (frame or tsv path, six columns) and ``sr_gwes_clust.png`` /
    ``sr_gwes_combi.png`` from ``sr_links`` (frame or tsv path, nine columns) in ``plt_folder`` (default ``PLOTS`` in the working directory).
    Grey ARACNE == 0 points lie under the direct ones, which are drawn by ascending ``srp_max`` (``are_srlinks_ordered``: in reverse row order).
    With ``engine`` and no ``sr_links`` the short-range figures are rendered from the engine's resident reduced table (after
    ``perform_MI_computation``), without a copy to the host; ``aracne=False`` for a table whose ARACNE step was skipped (``runARACNE=False``: every
    link is drawn as direct, like the frame's ARACNE column of ones) — with the default the library refuses such a table instead of guessing.
    ``reader="native"``: links given as paths are parsed on the device and never become a frame — the columns stay there, the facets come from
    ``torch.unique`` on the device, and the figures are rendered from the device columns.
    Returns the paths written."""
    from .engine import Engine
    from .links_io import check_reader
    native = check_reader(reader)
    if plt_folder is None:
        plt_folder = os.path.join(os.getcwd(), "PLOTS")
    lr_dev, sr_dev = native and lr_links is not None and _is_path(lr_links), native and sr_links is not None and _is_path(sr_links)
    lr = None if lr_links is None or lr_dev else _frame(lr_links, read_LongRangeLinks, 6, LR_COLS, LR_ERR)
    sr = None if sr_links is None or sr_dev else _frame(sr_links, read_ShortRangeLinks, 9, SR_COLS, SR_ERR)
    if lr_dev or sr_dev:
        return _make_gwes_plots_native(lr_links if lr_dev else None, lr, sr_links if sr_dev else None, sr, plt_folder, are_srlinks_ordered, engine, D)
    from_engine = sr is None and engine is not None
    if from_engine and are_srlinks_ordered:
        raise ValueError("are_srlinks_ordered needs the sr_links frame: the engine's resident table has no row order of its own")
    os.makedirs(plt_folder, exist_ok=True)
    own = engine is None and (lr is not None or sr is not None)
    eng = Engine(0) if own else engine
    out = {}
    try:
        if lr is not None:
            out["lr_gwes"] = os.path.join(plt_folder, "lr_gwes.png")
            render_scatter(eng, lr["len"].to_numpy(), lr["MI"].to_numpy(), opts=plot_opts(L.PLOT_LR, D, layer_rgb=(0, 0)), path=out["lr_gwes"])
        if sr is not None or from_engine:
            out["sr_gwes_clust"] = os.path.join(plt_folder, "sr_gwes_clust.png")
            out["sr_gwes_combi"] = os.path.join(plt_folder, "sr_gwes_combi.png")
        if sr is not None:
            panel, labels = sr_facets(sr["clust_c"].to_numpy())
            cols = (sr["len"].to_numpy(), sr["MI"].to_numpy(), sr["srp_max"].to_numpy(), (sr["ARACNE"].to_numpy() != 0).astype(np.uint8))
            render_scatter(eng, *cols, panel, opts=plot_opts(L.PLOT_SR_CLUST, D, are_srlinks_ordered), n_panels=max(len(labels), 1), labels=labels,
                           path=out["sr_gwes_clust"])
            render_scatter(eng, *cols, None, opts=plot_opts(L.PLOT_SR_COMBI, D, are_srlinks_ordered), path=out["sr_gwes_combi"])
        elif from_engine:
            render_links(eng, 0, opts=plot_opts(L.PLOT_SR_CLUST, D), use_aracne=bool(aracne), path=out["sr_gwes_clust"])
            render_links(eng, 0, opts=plot_opts(L.PLOT_SR_COMBI, D), use_aracne=bool(aracne), path=out["sr_gwes_combi"])
    finally:
        if own:
            eng.close()
    return out


def _sr_figures(eng, cols, panel, labels, D, ordered, out):
    render_scatter(eng, *cols, panel, opts=plot_opts(L.PLOT_SR_CLUST, D, ordered), n_panels=max(len(labels), 1), labels=labels, path=out["sr_gwes_clust"])
    render_scatter(eng, *cols, None, opts=plot_opts(L.PLOT_SR_COMBI, D, ordered), path=out["sr_gwes_combi"])


def _make_gwes_plots_native(lr_path, lr, sr_path, sr, plt_folder, ordered, engine, D) -> dict:
    """make_gwes_plots with at least one table read on the device.  A table's figures are rendered before the next file is read: the device
    columns alias the engine's one buffer."""
    from .engine import Engine
    os.makedirs(plt_folder, exist_ok=True)
    own = engine is None
    eng = Engine(0) if own else engine
    out = {}
    try:
        if lr_path is not None or lr is not None:
            out["lr_gwes"] = os.path.join(plt_folder, "lr_gwes.png")
            if lr_path is not None:
                c = _device_columns(eng, lr_path, "lr", 6, LR_ERR)
                x, y = c["len"], c["MI"]
            else:
                x, y = lr["len"].to_numpy(), lr["MI"].to_numpy()
            render_scatter(eng, x, y, opts=plot_opts(L.PLOT_LR, D, layer_rgb=(0, 0)), path=out["lr_gwes"])
        if sr_path is not None or sr is not None:
            out["sr_gwes_clust"] = os.path.join(plt_folder, "sr_gwes_clust.png")
            out["sr_gwes_combi"] = os.path.join(plt_folder, "sr_gwes_combi.png")
            if sr_path is not None:
                import torch
                c = _device_columns(eng, sr_path, "sr", 9, SR_ERR)
                panel, labels = sr_facets_device(c["clust_c"])
                cols = (c["len"], c["MI"], c["srp_max"], (c["ARACNE"] != 0).to(torch.uint8))
            else:
                panel, labels = sr_facets(sr["clust_c"].to_numpy())
                cols = (sr["len"].to_numpy(), sr["MI"].to_numpy(), sr["srp_max"].to_numpy(), (sr["ARACNE"].to_numpy() != 0).astype(np.uint8))
            _sr_figures(eng, cols, panel, labels, D, ordered, out)
    finally:
        if own:
            eng.close()
    return out
