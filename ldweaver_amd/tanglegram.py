"""The tanglegrams of the reference (R/createTanglegram.R:26-296): the top hits cut into ``break_segments`` stretches of the genome, and for every
stretch the links between gene regions drawn between two copies of that stretch.  DESIGN.md 24.

The SELECTION is the reference's, step by step: which rows go into which file (``tanglegram_segments``), the grouping by gene pair with the maximum
weight (``tanglegram_links``), where a locus lies (``locus_ranges``) and which links are dropped.  The three frames of a segment (``chr``, ``ann``,
``links``) are what the reference hands to chromoMap.  The PICTURE is ours (chromoMap's HTML widget is not imitated): an integer layout
(``tanglegram_layout``), the links as translucent capsules under opaque rectangles for the bars and the loci (``tanglegram_marks``), rendered on the
device (``ldw_plot_tanglegram``), the labels drawn by the host.  Names are matched LITERALLY (R's ``grep`` takes them as regular expressions)."""
from __future__ import annotations

import heapq
import os
import warnings

import numpy as np

from .network import ARC_SEGMENTS, _half_up, pair_counts, text_scale

RGB_BAR = 0xBEBEBE      # R's "grey"
RGB_LOCUS = 0x4682B4    # "steelblue"
RGB_LINK = 0xEE0000     # R's "red2" (links.colors, :282)
BAR_H = 12              # bar height in text-scale units
MIN_GAP = 64            # pixels between the bars, at least


# ---- the segments (:35-49) ------------------------------------------------------------------------------------------------------------------------

def complete_linkage_1d(pos, k):
    """``cutree(hclust(dist(pos)), k)`` for points of a line: under complete linkage the two closest clusters are always neighbouring intervals of the
    sorted points, so the neighbouring pair of smallest span (max of the right minus min of the left) is merged until k intervals are left.  Among pairs
    of equal span the LEFTMOST is merged (our tie rule; R's order among ties is not restated).  Equal positions keep their row order (stable sort).
    Returns the labels 1, 2, ... in order of first appearance by row, as ``cutree`` gives them."""
    v = np.asarray(pos, dtype=np.float64)
    n = len(v)
    order = np.argsort(v, kind="stable")
    sv = v[order]
    hi = list(range(n))            # interval i (named by its first sorted index) is sorted indices i .. hi[i]
    nxt = list(range(1, n + 1))    # the interval to its right (n: none)
    prv = list(range(-1, n - 1))   # the interval to its left (-1: none)
    alive = [True] * n
    heap = [(sv[i + 1] - sv[i], i, i + 1, i + 1) for i in range(n - 1)]
    heapq.heapify(heap)
    left = n
    while left > k:
        _, a, b, hb = heapq.heappop(heap)
        if not (alive[a] and alive[b] and nxt[a] == b and hi[b] == hb):
            continue               # (an entry of intervals that have changed since)
        hi[a], nxt[a], alive[b] = hi[b], nxt[b], False
        left -= 1
        c, p = nxt[a], prv[a]
        if c < n:
            prv[c] = a
            heapq.heappush(heap, (sv[hi[c]] - sv[a], a, c, hi[c]))
        if p >= 0:                 # the pair to the left of a: its span grew with a
            heapq.heappush(heap, (sv[hi[a]] - sv[p], p, a, hi[a]))
    cluster = np.zeros(n, dtype=np.int64)      # per row: the first sorted index of its interval
    for a in range(n):
        if alive[a]:
            cluster[order[a:hi[a] + 1]] = a
    first = {}
    out = np.zeros(n, dtype=np.int64)
    for r in range(n):
        out[r] = first.setdefault(int(cluster[r]), len(first) + 1)
    return out


def tanglegram_segments(pos1, break_segments=5):
    """The file number of every row (:35-49) and the left-to-right rank of every file number.  The relabelling loop of the reference is restated AS IT
    STANDS: with ``ord = order(min pos1 per cluster)`` the original cluster i becomes ``ord[i]`` — the permutation itself, not its inverse — so when
    ``ord`` is a 3-cycle, ``tng_2`` is not the second stretch from the left.  Returns (seg int64 [rows] in 1..k, rank int64 [k]: rank[j - 1] = the
    position from the left, 1-based, of the stretch in file j)."""
    v = np.asarray(pos1, dtype=np.float64).ravel()
    k = int(break_segments)
    if len(v) < 2:
        raise ValueError("tophits needs at least 2 rows")
    if k != break_segments or not 1 <= k <= 10:
        raise ValueError("break_segments must be an integer in 1..10")
    if k > len(v):
        raise ValueError(f"{k} segments for {len(v)} rows")
    if not np.all(np.isfinite(v)):
        raise ValueError("pos1 holds a missing or non-finite position")
    lab = complete_linkage_1d(v, k)
    mins = np.asarray([np.min(v[lab == i]) for i in range(1, k + 1)])
    ord_ = np.argsort(mins, kind="stable") + 1                    # :38
    seg = ord_[lab - 1]                                            # :41-49
    rank = np.zeros(k, dtype=np.int64)
    for r, i in enumerate(ord_):                                   # original cluster i is the r-th from the left and lies in file ord[i]
        rank[ord_[i - 1] - 1] = r + 1
    return seg.astype(np.int64), rank


# ---- the links of a segment (:60-82) ---------------------------------------------------------------------------------------------------------------

def _missing(x):
    return not isinstance(x, str) or x == ""      # (None, NaN, NA: a region name is a string)


def weight_column(links_type):
    if links_type == "SR":
        return "srp"
    if links_type == "LR":
        return "MI"
    raise ValueError("Links type must be SR or LR")


def tanglegram_links(p1, p2, w):
    """:62-82 for the rows of one segment: the distinct ordered pairs (p1a, p2a) sorted by code point (``network.pair_counts``), each with the maximum
    weight of its rows, and ``all_locs`` = the distinct names of p1a followed by p2a in first-appearance order.  Rows with a missing or empty region
    name are dropped with a warning (R would group NA).  Returns (p1a, p2a, w float64, all_locs)."""
    p1, p2, w = list(p1), list(p2), np.asarray(w, dtype=np.float64)
    keep = [i for i in range(len(p1)) if not (_missing(p1[i]) or _missing(p2[i]))]
    if len(keep) != len(p1):
        warnings.warn(f"{len(p1) - len(keep)} rows without a gene region name are left out of the tanglegram", UserWarning, stacklevel=2)
    a, b, wk = [str(p1[i]) for i in keep], [str(p2[i]) for i in keep], w[keep]
    u1, u2, _ = pair_counts(a, b)                                  # :74
    an, bn = np.asarray(a, dtype=object), np.asarray(b, dtype=object)
    uw = np.asarray([np.max(wk[(an == x) & (bn == y)]) for x, y in zip(u1, u2)], dtype=np.float64)     # :76-77 (:78-79 change nothing)
    return u1, u2, uw, list(dict.fromkeys(u1 + u2))               # :82


# ---- where a locus lies (:84-159) ----------------------------------------------------------------------------------------------------------------

def _first_match(needle, hay):
    for i, s in enumerate(hay):
        if isinstance(s, str) and needle in s:
            return i
    return -1


def locus_ranges(all_locs, gbk=None, gff=None):
    """Start and end of every name, by LITERAL substring search.  ``gbk``: the first CDS row whose locus_tag contains the name, and that row's own
    start and end (the reference walks five feature tables of genbankr and reads the coordinates from its ``genes`` table; our record holds the CDS
    rows).  ``gff``: every ``GENE_`` stripped from the name (:147), the first row of ``gff.gff`` whose attributes contain the rest.  A name that
    matches nothing gets the reference's warning and the range None; for ``gff`` every name is tested, as in the ``gbk`` branch (the reference's test
    sits outside its loop and sees the last name only).  Returns (ranges: list of (start, end) or None, not_found: names)."""
    if (gbk is None) == (gff is None):
        raise ValueError("Provide either one of gbk or gff")
    if gbk is not None:
        rec = gbk["gbk"] if isinstance(gbk, dict) else gbk
        tab, hay = rec.cds, list(rec.cds["locus_tag"])
    else:
        tab, hay = gff.gff, list(gff.gff["attributes"])
    st, en = np.asarray(tab["start"], dtype=np.int64), np.asarray(tab["end"], dtype=np.int64)
    ranges, not_found = [], []
    for name in all_locs:
        i = _first_match(name if gbk is not None else name.replace("GENE_", ""), hay)
        if i < 0:
            warnings.warn(f"Could not locate {name} in the genbankr parsed gbk file, these link will be dropped from the tanglegram...", UserWarning, stacklevel=2)
            not_found.append(name)
            ranges.append(None)
        else:
            ranges.append((int(st[i]), int(en[i])))
    return ranges, not_found


def segment_frames(p1a, p2a, w, all_locs, ranges):
    """chromoMap's three inputs (:264-276): ``chr`` (p and q from min(start) - 1000 to max(end) + 1000), ``ann`` (every locus on both bars) and
    ``links`` (p_<p1a>, 1, q_<p2a>, 1, and the weight)."""
    import pandas as pd
    n = len(all_locs)
    st, en = [r[0] for r in ranges], [r[1] for r in ranges]
    chr_ = pd.DataFrame({"V1": ["p", "q"] if n else [], "V2": np.asarray([min(st) - 1000] * 2 if n else [], dtype=np.int64),
                         "V3": np.asarray([max(en) + 1000] * 2 if n else [], dtype=np.int64)})
    ann = pd.DataFrame({"V1": ["p_" + s for s in all_locs] + ["q_" + s for s in all_locs], "V2": ["p"] * n + ["q"] * n, "V3": np.asarray(st + st, dtype=np.int64),
                        "V4": np.asarray(en + en, dtype=np.int64)})
    links = pd.DataFrame({"V1": ["p_" + s for s in p1a], "V2": np.ones(len(p1a), dtype=np.int64), "V3": ["q_" + s for s in p2a],
                          "V4": np.ones(len(p1a), dtype=np.int64), "w": np.asarray(w, dtype=np.float64)})
    return chr_, ann, links


# ---- the picture (ours) ------------------------------------------------------------------------------------------------------------------------------

def tanglegram_layout(v2, v3, all_locs, ranges, plot_w, plot_h, segment=1):
    """OUR layout, integers only.  s = text_scale(plot_w); mx = plot_w // 20, PW = plot_w - 2 mx, x(c) = mx + ((c - V2)(PW - 1)) // (V3 - V2); bars 12 s
    high, the p bar's top at yp = 24 s + Lmax and the q bar's at yq = plot_h - 18 s - Lmax, Lmax = (6 len - 1) s of the longest label.  A locus is
    [x(start), x(end) + 1) on the bar's rows, its centre xc = (x(start) + x(end)) // 2.  Labels read upwards, 7 s wide with the left edge xc - (7 s) // 2,
    ending 2 s above the p bar and starting 2 s below the q bar.  Walking the loci by ascending (xc, index), a label with fewer than s free columns
    between its left edge and the last drawn label is skipped (drawn = False: the host gets an empty string and reports a box with w = 0).
    Returns a dict: s, mx, PW, yp, yq, bar_h, x0 / x1 / xc (int64 per locus), drawn (bool per locus), label_xy (int32 [2 n, 2]: the anchors = bottom-left
    corners of the turned texts, p labels then q labels), label_box (int32 [2 n, 4]: x, y, w, h as the host reports them) and title."""
    plot_w, plot_h, v2, v3 = int(plot_w), int(plot_h), int(v2), int(v3)
    if not (64 <= plot_w <= 8192 and 64 <= plot_h <= 8192):
        raise ValueError("plot_w and plot_h must lie in 64..8192 pixels")
    if v3 <= v2:
        raise ValueError(f"the segment's range {v2}..{v3} is empty")
    s = text_scale(plot_w)
    n = len(all_locs)
    mx = plot_w // 20
    pw = plot_w - 2 * mx
    lmax = max([(6 * len(t) - 1) * s for t in all_locs if t] + [0])
    bar_h = BAR_H * s
    yp, yq = 24 * s + lmax, plot_h - 18 * s - lmax
    if yq - (yp + bar_h) < MIN_GAP:
        raise ValueError(f"a canvas {plot_h} pixels high leaves {yq - (yp + bar_h)} pixels between the bars ({MIN_GAP} at least): labels of {lmax} pixels")

    def x(c):
        return mx + ((int(c) - v2) * (pw - 1)) // (v3 - v2)

    xs, xe = [x(r[0]) for r in ranges], [x(r[1]) for r in ranges]
    x0 = np.asarray([min(a, b) for a, b in zip(xs, xe)], dtype=np.int64)
    x1 = np.asarray([max(a, b) + 1 for a, b in zip(xs, xe)], dtype=np.int64)
    xc = np.asarray([(a + b) // 2 for a, b in zip(xs, xe)], dtype=np.int64)
    drawn = np.zeros(n, dtype=bool)
    last_right = None                                  # one past the last drawn label's columns
    for i in sorted(range(n), key=lambda i: (int(xc[i]), i)):
        lx = int(xc[i]) - (7 * s) // 2
        if all_locs[i] and (last_right is None or lx - last_right >= s):
            drawn[i] = True
            last_right = lx + 7 * s
    xy = np.zeros((2 * n, 2), dtype=np.int32)
    box = np.zeros((2 * n, 4), dtype=np.int32)
    for i in range(n):
        lx, tw = int(xc[i]) - (7 * s) // 2, (6 * len(all_locs[i]) - 1) * s if all_locs[i] else 0
        xy[i] = (lx, yp - 2 * s - 1)                   # the p label's bottom row: 2 s free rows above the bar
        xy[n + i] = (lx, yq + bar_h + 2 * s + tw - 1)  # the q label's top row: 2 s free rows below the bar
        for k in (i, n + i):
            box[k] = (xy[k, 0], xy[k, 1] - tw + 1, 7 * s, tw) if drawn[i] else (xy[k, 0], xy[k, 1], 0, 0)
    return dict(s=s, mx=mx, PW=pw, yp=yp, yq=yq, bar_h=bar_h, x0=x0, x1=x1, xc=xc, drawn=drawn, label_xy=xy, label_box=box,
                title=f"Tanglegram {segment}: {v2} - {v3} bp", plot_w=plot_w, plot_h=plot_h)


def link_polyline(a, b):
    """The link from pixel a (under the p bar) to pixel b (over the q bar): the cubic Bezier curve whose control points lie a third of the gap below a and a
    third of the gap above b, flattened to ARC_SEGMENTS segments with vertices rounded half up and both ends exact: int32 [ARC_SEGMENTS + 1, 2]."""
    ax, ay, bx, by = float(a[0]), float(a[1]), float(b[0]), float(b[1])
    gap = by - ay
    c1y, c2y = ay + gap / 3.0, by - gap / 3.0
    pts = np.zeros((ARC_SEGMENTS + 1, 2), dtype=np.int32)
    for i in range(ARC_SEGMENTS + 1):
        t = i / ARC_SEGMENTS
        u = 1 - t
        pts[i] = (_half_up(u ** 3 * ax + 3 * u * u * t * ax + 3 * u * t * t * bx + t ** 3 * bx),
                  _half_up(u ** 3 * ay + 3 * u * u * t * c1y + 3 * u * t * t * c2y + t ** 3 * by))
    pts[0], pts[-1] = (int(a[0]), int(a[1])), (int(b[0]), int(b[1]))
    return pts


def tanglegram_marks(lay, p1a, p2a, w, all_locs):
    """The marks of one segment.  Rectangles in list order: the p bar, the q bar (RGB_BAR), the loci of p, then of q (RGB_LOCUS), in ``all_locs`` order.
    One link per pair from (xc(p1a), yp + 12 s) to (xc(p2a), yq - 1) as ARC_SEGMENTS capsules, width 1 + round(2 s w') and alpha round(64 + 191 w') with
    w' = w / max w (non-finite: 0; clipped to 0..1), colour RGB_LINK; drawn in ascending w', ties in pair order: the strongest link on top.
    Returns (capsules ``Engine.CAPSULE``, rects ``Engine.RECT``)."""
    from .engine import Engine
    n, s, yp, yq, bar_h = len(all_locs), lay["s"], lay["yp"], lay["yq"], lay["bar_h"]
    rects = np.zeros(2 + 2 * n, dtype=Engine.RECT)
    rects[0] = (lay["mx"], yp, lay["mx"] + lay["PW"], yp + bar_h, RGB_BAR)
    rects[1] = (lay["mx"], yq, lay["mx"] + lay["PW"], yq + bar_h, RGB_BAR)
    for i in range(n):
        rects[2 + i] = (lay["x0"][i], yp, lay["x1"][i], yp + bar_h, RGB_LOCUS)
        rects[2 + n + i] = (lay["x0"][i], yq, lay["x1"][i], yq + bar_h, RGB_LOCUS)
    w = np.asarray(w, dtype=np.float64)
    with np.errstate(all="ignore"):
        wn = w / np.max(w) if len(w) else w
    wn = np.clip(np.where(np.isfinite(wn), wn, 0.0), 0.0, 1.0)
    index = {t: i for i, t in enumerate(all_locs)}
    caps = np.zeros(len(w) * ARC_SEGMENTS, dtype=Engine.CAPSULE)
    k = 0
    for j in np.argsort(wn, kind="stable"):
        wt = float(wn[j])
        pts = link_polyline((lay["xc"][index[p1a[j]]], yp + bar_h), (lay["xc"][index[p2a[j]]], yq - 1))
        for i in range(ARC_SEGMENTS):
            caps[k] = (pts[i, 0], pts[i, 1], pts[i + 1, 0], pts[i + 1, 1], 1 + _half_up(2 * s * wt), RGB_LINK, min(255, max(1, _half_up(64 + 191 * wt))))
            k += 1
    return caps, rects


# ---- the stage function -----------------------------------------------------------------------------------------------------------------------------

def create_tanglegram(tophits, gbk=None, gff=None, tanglegram_folder=None, break_segments=5, links_type="SR", plot_w=6000, plot_h=2400, *, engine=None):
    """``create_tanglegram`` (R/createTanglegram.R:26-296).  Returns one dict per file number 1..break_segments: ``segment``, ``rank`` (its stretch's place
    from the left), the frames ``chr``, ``ann``, ``links`` (chromoMap's inputs), ``capsules``, ``rects``, ``labels`` (text, xy, drawn) and, with
    ``tanglegram_folder``, ``png`` (``tng_<segment>.png``) and ``boxes`` (what the host drew: the labels, p then q, and the title).  A segment whose
    links all name loci that are not found gets a warning, empty frames and no file.  The pictures need a GPU; without a folder nothing is drawn and
    none is needed."""
    if (gbk is None) == (gff is None):                      # :27
        raise ValueError("Provide either one of gbk or gff")
    wcol = weight_column(links_type)                        # :61-71
    plot_w, plot_h = int(plot_w), int(plot_h)
    if not (64 <= plot_w <= 8192 and 64 <= plot_h <= 8192):
        raise ValueError("plot_w and plot_h must lie in 64..8192 pixels")
    seg, rank = tanglegram_segments(tophits["pos1"], break_segments)
    g1, g2, wt = list(tophits["pos1_genreg"]), list(tophits["pos2_genreg"]), np.asarray(tophits[wcol], dtype=np.float64)
    from .engine import Engine
    out, eng = [], engine
    try:
        for c in range(1, int(break_segments) + 1):         # :59
            rows = np.nonzero(seg == c)[0]
            p1a, p2a, w, all_locs = tanglegram_links([g1[i] for i in rows], [g2[i] for i in rows], wt[rows])
            ranges, not_found = locus_ranges(all_locs, gbk, gff) if all_locs else ([], [])
            if not_found:                                   # :163-174
                gone = set(not_found)
                keep = [i for i in range(len(p1a)) if p1a[i] not in gone and p2a[i] not in gone]
                p1a, p2a, w = [p1a[i] for i in keep], [p2a[i] for i in keep], w[keep]
                place = dict(zip(all_locs, ranges))
                all_locs = list(dict.fromkeys(p1a + p2a))
                ranges = [place[t] for t in all_locs]
            chr_, ann, links = segment_frames(p1a, p2a, w, all_locs, ranges)
            res = dict(segment=c, rank=int(rank[c - 1]), chr=chr_, ann=ann, links=links, capsules=np.zeros(0, dtype=Engine.CAPSULE),
                       rects=np.zeros(0, dtype=Engine.RECT), labels=dict(text=[], xy=np.zeros((0, 2), dtype=np.int32), drawn=np.zeros(0, dtype=bool)))
            out.append(res)
            if not p1a:
                warnings.warn(f"Tanglegram {c} has no link left: no file is written", UserWarning, stacklevel=2)
                continue
            lay = tanglegram_layout(chr_["V2"][0], chr_["V3"][0], all_locs, ranges, plot_w, plot_h, c)
            caps, rects = tanglegram_marks(lay, p1a, p2a, w, all_locs)
            drawn2 = np.concatenate([lay["drawn"], lay["drawn"]])
            res.update(capsules=caps, rects=rects, labels=dict(text=all_locs + all_locs, xy=lay["label_xy"], drawn=drawn2), title=lay["title"], layout=lay)
            if tanglegram_folder is not None:
                if eng is None:
                    eng = Engine(0)
                os.makedirs(tanglegram_folder, exist_ok=True)          # :32
                path = os.path.join(str(tanglegram_folder), f"tng_{c}.png")
                texts = [t if d else "" for t, d in zip(all_locs + all_locs, drawn2)]
                _, boxes = eng.plot_tanglegram(caps, rects, plot_w, plot_h, lay["label_xy"], texts, lay["title"], lay["s"], png_path=path)
                res["png"] = path
                res["boxes"] = boxes
    finally:
        if eng is not None and engine is None:
            eng.close()
    return out
