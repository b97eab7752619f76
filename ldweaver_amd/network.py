"""The gene networks of the reference (R/createNetworkPlot.R): ``create_network_for_gene`` collects the annotated links of one gene (and, at
level 2, of its neighbours) from ``sr_links_annotated.tsv`` / ``lr_links_annotated.tsv``; ``create_network`` turns such a frame (or a tophits
frame) into the edge list of the gene graph and draws it.  DESIGN.md 22.

The file search runs on the device (``Engine.links_grep``: include/ldweaver_amd.h 14) or, with ``reader="pandas"``, through pandas; both match
the gene name LITERALLY (R's ``grep`` takes it as a regular expression: a name with metacharacters is matched as text here).  The edge list is
the reference's, step by step; the picture is ours: a deterministic layout in integer pixels, the edges rendered on the device as translucent
capsules (``ldw_plot_network``), the labels drawn by the host."""
from __future__ import annotations

import csv
import math

import numpy as np

from .links_io import check_reader

FRAME_COLS = ["pos1", "pos2", "pos1_ann", "pos2_ann", "MI", "links", "ARACNE"]       # R/createNetworkPlot.R:183-189
_NUM = ("pos1", "pos2", "len", "ARACNE", "MI")
_STR = ("pos1_ann", "pos2_ann", "links")
MAX_NEEDLES = 1024
ARC_SEGMENTS = 16


# ---- the frame of matching rows ---------------------------------------------------------------------------------------------------------------

def _num_col(v):
    """float64 values as int64 where every one is a finite integer below 2^53 (what read.table / pandas make of an integer column)."""
    v = np.asarray(v, dtype=np.float64)
    if len(v) and np.all(np.isfinite(v)) and np.all(v == np.floor(v)) and np.all(np.abs(v) < 2.0 ** 53):
        return v.astype(np.int64)
    return v


def _frame(pos1, pos2, a1, a2, mi, links, aracne):
    import pandas as pd
    return pd.DataFrame({"pos1": np.asarray(pos1, dtype=np.float64), "pos2": np.asarray(pos2, dtype=np.float64), "pos1_ann": np.asarray(a1, dtype=object),
                         "pos2_ann": np.asarray(a2, dtype=object), "MI": np.asarray(mi, dtype=np.float64), "links": np.asarray(links, dtype=object),
                         "ARACNE": np.asarray(aracne, dtype=np.float64)}, columns=FRAME_COLS)


def _empty():
    return _frame([], [], [], [], [], [], [])


def _bind(parts):
    """rbind (:209, :272): frames without rows add nothing."""
    import pandas as pd
    parts = [p for p in parts if len(p)]
    return pd.concat(parts, ignore_index=True) if parts else _empty()


def _finish(df):
    """duplicated() keeps the first occurrence (:284-285); the integer columns get their integer type."""
    df = df[~df.duplicated()].reset_index(drop=True)
    for c in ("pos1", "pos2", "ARACNE"):
        df[c] = _num_col(df[c].to_numpy())
    return df


def _filters(df, drop_syXsy, drop_indirect):
    if drop_syXsy:                       # :212-215
        df = df[df["links"] != "syXsy"]
    if drop_indirect:                    # :216
        df = df[df["ARACNE"] == 1]
    return df.reset_index(drop=True)


def first_token(s, separator):
    """``unlist(strsplit(x, separator))[1]`` (:51) with a literal separator."""
    return s.split(separator)[0] if separator else s


def pair_counts(p1a, p2a):
    """``plyr::ddply(df, .(p1a, p2a), nrow)`` (:60): the distinct ordered pairs, sorted by p1a then p2a (code-point order; R sorts by the session's
    collation), with their row counts."""
    cnt = {}
    for a, b in zip(p1a, p2a):
        cnt[(a, b)] = cnt.get((a, b), 0) + 1
    keys = sorted(cnt)
    return [k[0] for k in keys], [k[1] for k in keys], [cnt[k] for k in keys]


def neighbour_genes(df, gene_name, separator, min_links_to_include):
    """The level-2 genes of :220-239 from the filtered level-1 rows.  avail_links starts at nrow, so the loop of :224-234 runs once over all rows.
    ``genes[-which(genes == gene_name)]``: when gene_name is no node name, ``-integer(0)`` selects nothing and NO gene is left."""
    p1a = [first_token(s, separator) for s in df["pos1_ann"]]
    p2a = [first_token(s, separator) for s in df["pos2_ann"]]
    u1, u2, v1 = pair_counts(p1a, p2a)
    keep = [k for k in range(len(v1)) if v1[k] >= min_links_to_include]     # :236
    genes = list(dict.fromkeys([u1[k] for k in keep] + [u2[k] for k in keep]))   # :238
    if gene_name not in genes:
        return []
    return [g for g in genes if g != gene_name]     # :239


def _read_pandas(path):
    import pandas as pd
    return pd.read_csv(path, sep="\t", header=0, quoting=csv.QUOTE_NONE, dtype={c: str for c in _STR}, keep_default_na=False,
                       na_values={c: ["NA", "NaN", "nan"] for c in _NUM}, float_precision="round_trip")


def _match_pandas(tab, gene):
    hit = tab["pos1_ann"].str.contains(gene, regex=False) | tab["pos2_ann"].str.contains(gene, regex=False)     # :180
    t = tab[hit.to_numpy()]
    return _frame(t["pos1"], t["pos2"], t["pos1_ann"], t["pos2_ann"], t["MI"], t["links"], t["ARACNE"])


def _dec(b):
    return b.decode("utf-8", "surrogateescape")


def _grep_frame(res, sel=None):
    idx = range(len(res["row"])) if sel is None else sel
    num = res["num"]
    return _frame([num[i, 0] for i in idx], [num[i, 1] for i in idx], [_dec(res["pos1_ann"][i]) for i in idx], [_dec(res["pos2_ann"][i]) for i in idx],
                  [num[i, 4] for i in idx], [_dec(res["links"][i]) for i in idx], [num[i, 3] for i in idx])


def create_network_for_gene(gene_name, sr_annotated_path=None, lr_annotated_path=None, drop_syXsy=True, drop_indirect=True, level=1, separator=":",
                            min_links_to_include=3, *, engine=None, reader="native", chunk_bytes=0):
    """``create_network_for_gene`` (R/createNetworkPlot.R:169-290): the frame ``pos1 pos2 pos1_ann pos2_ann MI links ARACNE`` of the links whose
    annotation names ``gene_name`` — level 2: and those of the genes linked to it at least ``min_links_to_include`` times — with the reference's
    rows in the reference's order.  ``reader="native"`` searches the files on the device (one pass per file and level), ``"pandas"`` reads them
    whole; the results are equal.  No matching row gives an empty frame."""
    if sr_annotated_path is None and lr_annotated_path is None:     # :174
        raise ValueError("<sr> or <lr> annotated_link tsv file path must be provided!")
    if level != 1 and level != 2:                                   # :175
        raise ValueError("Level must be 1 or 2")
    if not isinstance(gene_name, str) or not 1 <= len(gene_name.encode("utf-8", "surrogateescape")) <= 255:
        raise ValueError("gene_name must be a string of 1..255 bytes")
    native = check_reader(reader)
    paths = [p for p in (sr_annotated_path, lr_annotated_path) if p is not None]     # sr before lr (:209)
    if not native:
        tabs = [_read_pandas(p) for p in paths]
        df = _bind([_match_pandas(t, gene_name) for t in tabs])
        df = _filters(df, drop_syXsy, drop_indirect)
        if level == 2 and len(df):
            parts = [df]
            for gene in neighbour_genes(df, gene_name, separator, min_links_to_include):     # :241-273
                parts += [_match_pandas(t, gene) for t in tabs]
            df = _filters(_bind(parts), drop_syXsy, drop_indirect)     # :275-280
        return _finish(df)
    from .engine import Engine
    own = engine is None
    eng = Engine(0) if own else engine
    try:
        # (the row-wise filters commute with the row binding of :209 and :272: the device applies them while it searches)
        df = _bind([_grep_frame(eng.links_grep(p, [gene_name], drop_syXsy, drop_indirect, chunk_bytes)) for p in paths])
        if level == 2 and len(df):
            genes = neighbour_genes(df, gene_name, separator, min_links_to_include)
            for g in genes:
                if not 1 <= len(g.encode("utf-8", "surrogateescape")) <= 255:
                    raise ValueError(f"the neighbour gene name {g!r} has no bytes or more than 255: use reader='pandas'")
            parts = [df]
            for lo in range(0, len(genes), MAX_NEEDLES):
                batch = genes[lo:lo + MAX_NEEDLES]
                found = [eng.links_grep(p, batch, drop_syXsy, drop_indirect, chunk_bytes) for p in paths]
                for j in range(len(batch)):        # the reference's order: per gene, its sr rows, then its lr rows, each in file order
                    w, bit = j >> 6, np.uint64(1) << np.uint64(j & 63)
                    for res in found:
                        sel = np.nonzero(res["mask"][:, w] & bit)[0] if len(res["row"]) else []
                        if len(sel):
                            parts.append(_grep_frame(res, sel))
            df = _bind(parts)
        return _finish(df)
    finally:
        if own:
            eng.close()


# ---- the edge list ------------------------------------------------------------------------------------------------------------------------------

def network_edges(tophits, separator=":", max_plot_nodes=None, min_links_to_include=2):
    """R/createNetworkPlot.R:36-118 on the host: the frame ``p1 p2 Num_Links weights``.  One deviation: where the reference indexes past the last
    row (max_plot_nodes > nrow: an NA group that its loop filter drops again) the rows are clamped."""
    import pandas as pd
    n = len(tophits)
    if n == 0:
        raise ValueError("tophits has no rows")
    ann1, ann2, mi = list(tophits["pos1_ann"]), list(tophits["pos2_ann"]), np.asarray(tophits["MI"], dtype=np.float64)
    if max_plot_nodes is None:      # :40-45
        avail = max_nodes = n
    else:
        avail = max_nodes = int(max_plot_nodes)
        if max_nodes < 1:
            raise ValueError("max_plot_nodes must be at least 1")
    while True:                     # :49-65
        k = min(avail, n)
        p1a = [first_token(s, separator) for s in ann1[:k]]
        p2a = [first_token(s, separator) for s in ann2[:k]]
        w = mi[:k]
        u1, u2, v1 = pair_counts(p1a, p2a)
        stop = len(u1) >= max_nodes
        avail += 1
        if avail > n:
            stop = True
        if stop:
            break
    keep = [i for i in range(len(v1)) if v1[i] >= min_links_to_include]     # :67
    u1, u2, v1 = [u1[i] for i in keep], [u2[i] for i in keep], [v1[i] for i in keep]
    p1a, p2a = np.asarray(p1a, dtype=object), np.asarray(p2a, dtype=object)
    uw = [float(np.max(w[(p1a == a) & (p2a == b)])) for a, b in zip(u1, u2)]     # :70-72
    in_p2 = set(u2)                 # :75-80
    for i in [i for i in range(len(u1)) if u1[i] in in_p2]:
        u1[i], u2[i] = u2[i], u1[i]
    in_p1 = set(u1)                 # :82-87
    for i in [i for i in range(len(u1)) if u2[i] in in_p1]:
        u1[i], u2[i] = u2[i], u1[i]
    pst1 = [a + " " + b for a, b in zip(u1, u2)]      # :91-106
    pst2 = set(b + " " + a for a, b in zip(u1, u2))
    for i in [i for i in range(len(pst1)) if pst1[i] in pst2]:
        mrg = pst1[i].split(" ")
        if len(mrg) < 2:
            continue
        l1 = [j for j in range(len(u1)) if u1[j] == mrg[0] and u2[j] == mrg[1]]
        l2 = [j for j in range(len(u1)) if u1[j] == mrg[1] and u2[j] == mrg[0]]
        if len(l1) == 1 and len(l2) == 1:
            a, b = l1[0], l2[0]
            v1[a] = v1[a] + v1[b]
            uw[a] = max(uw[a], uw[b])
            for col in (u1, u2, v1, uw):
                del col[b]
    kps = [i for i in range(len(u1)) if u1[i] != u2[i]]     # :109-117
    if not kps:
        raise ValueError("Everything is a loop!")
    sw = np.asarray([uw[i] for i in kps], dtype=np.float64)
    return pd.DataFrame({"p1": [u1[i] for i in kps], "p2": [u2[i] for i in kps], "Num_Links": np.asarray([v1[i] for i in kps], dtype=np.int64),
                         "weights": sw / np.max(sw)})       # :118


# ---- the picture ----------------------------------------------------------------------------------------------------------------------------------

def hue_palette(n):
    """``scales::hue_pal()(n)``: hcl(h = 15 + 360 (k - 1) / n, c = 100, l = 65), k = 1..n, as 0xRRGGBB — polar CIE-LUV (D65) to sRGB, channels
    clipped to [0, 1] and rounded to 8 bits."""
    out = []
    xn, yn, zn = 95.047, 100.0, 108.883
    un, vn = 4 * xn / (xn + 15 * yn + 3 * zn), 9 * yn / (xn + 15 * yn + 3 * zn)
    for k in range(n):
        h = math.radians(15.0 + 360.0 * k / n)
        l, c = 65.0, 100.0
        u, v = c * math.cos(h), c * math.sin(h)
        y = yn * ((l + 16.0) / 116.0) ** 3
        up, vp = u / (13 * l) + un, v / (13 * l) + vn
        x = 9.0 * y * up / (4.0 * vp)
        z = (12.0 - 3.0 * up - 20.0 * vp) * y / (4.0 * vp)
        lin = (3.240479 * x - 1.537150 * y - 0.498535 * z, -0.969256 * x + 1.875992 * y + 0.041556 * z, 0.055648 * x - 0.204043 * y + 1.057311 * z)
        rgb = 0
        for t in lin:
            t /= 100.0
            s = 1.055 * t ** (1 / 2.4) - 0.055 if t > 0.0031308 else 12.92 * t
            rgb = rgb << 8 | int(math.floor(255.0 * min(max(s, 0.0), 1.0) + 0.5))
        out.append(rgb)
    return out


def _half_up(v):
    return int(math.floor(v + 0.5))


def network_layout(edges, plot_w, plot_h):
    """OUR layout (igraph's "nicely" starts from random positions and is not imitated).  Nodes in order of first appearance in the edge list read row by
    row (p1, p2 of edge 0, of edge 1, ...).  Connected components by decreasing node count (ties: the component whose first node appears first) go
    row by row into a grid of cols = ceil(sqrt(ncomp * w / h)) by ceil(ncomp / cols) equal cells inside the margins (w / 20 left and right, h / 10
    top, h / 8 bottom).  A component's m nodes sit on the circle of radius 0.38 min(cell w, cell h) round the cell's centre, node k at the angle
    -pi / 2 + 2 pi k / m (from the top, clockwise), rounded half up to pixels; a component of two nodes sits on the horizontal diameter.
    Returns (names, xy int32 [nodes, 2], component of every node)."""
    names = list(dict.fromkeys(x for a, b in zip(edges["p1"], edges["p2"]) for x in (a, b)))
    index = {s: i for i, s in enumerate(names)}
    parent = list(range(len(names)))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for a, b in zip(edges["p1"], edges["p2"]):
        ra, rb = find(index[a]), find(index[b])
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    comps = {}
    for i in range(len(names)):
        comps.setdefault(find(i), []).append(i)
    order = sorted(comps.values(), key=lambda c: (-len(c), c[0]))
    ncomp = len(order)
    cols = max(1, int(math.ceil(math.sqrt(ncomp * plot_w / plot_h))))
    cols = min(cols, ncomp)
    rows = (ncomp + cols - 1) // cols
    mx, top, bottom = plot_w / 20.0, plot_h / 10.0, plot_h / 8.0
    cw, ch = (plot_w - 2 * mx) / cols, (plot_h - top - bottom) / rows
    xy = np.zeros((len(names), 2), dtype=np.int32)
    comp_of = np.zeros(len(names), dtype=np.int32)
    for ci, comp in enumerate(order):
        cx, cy = mx + (ci % cols + 0.5) * cw, top + (ci // cols + 0.5) * ch
        r = 0.38 * min(cw, ch)
        m = len(comp)
        for k, node in enumerate(comp):
            if m == 2:
                x, y = cx + (r if k else -r), cy
            else:
                t = -math.pi / 2 + 2 * math.pi * k / m
                x, y = cx + r * math.cos(t), cy + r * math.sin(t)
            xy[node] = (min(max(_half_up(x), 0), plot_w - 1), min(max(_half_up(y), 0), plot_h - 1))
            comp_of[node] = ci
    return names, xy, comp_of


def edge_polyline(a, b, bend=0.15):
    """The arc from pixel a to pixel b: the quadratic Bezier curve through the control point mid + bend * perp(b - a), flattened to ARC_SEGMENTS
    segments with vertices rounded half up: int32 [ARC_SEGMENTS + 1, 2]."""
    ax, ay, bx, by = float(a[0]), float(a[1]), float(b[0]), float(b[1])
    cx, cy = (ax + bx) / 2 - bend * (by - ay), (ay + by) / 2 + bend * (bx - ax)
    pts = np.zeros((ARC_SEGMENTS + 1, 2), dtype=np.int32)
    for i in range(ARC_SEGMENTS + 1):
        t = i / ARC_SEGMENTS
        pts[i] = (_half_up((1 - t) ** 2 * ax + 2 * t * (1 - t) * cx + t * t * bx), _half_up((1 - t) ** 2 * ay + 2 * t * (1 - t) * cy + t * t * by))
    pts[0], pts[-1] = (int(a[0]), int(a[1])), (int(b[0]), int(b[1]))
    return pts


def text_scale(plot_w):
    return max(1, _half_up(plot_w / 1000.0))


def network_capsules(edges, names, xy, plot_w):
    """The capsule list of the edges, in edge order: colour by Num_Links (the k-th of the n distinct values ascending takes the k-th colour of
    ``hue_palette(n)``), width 1 + round(2 scale weights) pixels and alpha round(64 + 191 weights), scale = ``text_scale(plot_w)``.
    Returns (capsules, legend values, legend colours)."""
    from .engine import Engine
    index = {s: i for i, s in enumerate(names)}
    levels = sorted(set(int(v) for v in edges["Num_Links"]))
    pal = hue_palette(len(levels))
    sc = text_scale(plot_w)
    caps = np.zeros(len(edges) * ARC_SEGMENTS, dtype=Engine.CAPSULE)
    k = 0
    for a, b, nl, wt in zip(edges["p1"], edges["p2"], edges["Num_Links"], edges["weights"]):
        wt = float(wt) if np.isfinite(wt) else 0.0
        wt = min(max(wt, 0.0), 1.0)
        pts = edge_polyline(xy[index[a]], xy[index[b]])
        for i in range(ARC_SEGMENTS):
            caps[k] = (pts[i, 0], pts[i, 1], pts[i + 1, 0], pts[i + 1, 1], 1 + _half_up(2 * sc * wt), pal[levels.index(int(nl))], min(255, max(1, _half_up(64 + 191 * wt))))
            k += 1
    return caps, levels, pal


def create_network(tophits, netplot_path=None, plot_title=None, separator=":", max_plot_nodes=None, plot_w=6000, plot_h=4000, min_links_to_include=2, *,
                   engine=None):
    """``create_network`` (R/createNetworkPlot.R:28-144).  Returns a dict: ``edges`` (the frame p1 p2 Num_Links weights of :36-118), ``nodes`` (names in
    first-appearance order), ``node_xy`` (int32 pixel coordinates), ``capsules``, ``legend`` (Num_Links values and their colours) and, with
    ``netplot_path``, ``png`` (the path written) and ``boxes`` (what the host drew over the edge raster: node boxes, title, legend).  The picture needs a
    GPU; without a path nothing is drawn and none is needed."""
    if plot_title is None:      # :36
        plot_title = ""
    plot_w, plot_h = int(plot_w), int(plot_h)
    if not (64 <= plot_w <= 8192 and 64 <= plot_h <= 8192):
        raise ValueError("plot_w and plot_h must lie in 64..8192 pixels")
    edges = network_edges(tophits, separator, max_plot_nodes, min_links_to_include)
    names, xy, _ = network_layout(edges, plot_w, plot_h)
    caps, levels, pal = network_capsules(edges, names, xy, plot_w)
    out = dict(edges=edges, nodes=names, node_xy=xy, capsules=caps, legend=(levels, pal))
    if netplot_path is not None:
        from .engine import Engine
        own = engine is None
        eng = Engine(0) if own else engine
        try:
            _, boxes = eng.plot_network(caps, plot_w, plot_h, xy, names, plot_title, levels, pal, text_scale(plot_w), png_path=netplot_path)
        finally:
            if own:
                eng.close()
        out["png"] = str(netplot_path)
        out["boxes"] = boxes
    return out
