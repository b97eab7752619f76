"""Naive counterparts of ldweaver_amd/tree.py and of the device renderer of the tree view, written independently of both: a recursive-descent Newick
reader (small trees only), all-pairs patristic distances by brute force, a loop-by-loop transliteration of R/preptrees.R:67-179 over lists, and a
per-pixel painter of the two render rules of DESIGN.md 23 in Python integers."""
import math

import numpy as np


# ---- Newick, recursively ------------------------------------------------------------------------------------------------------------------------------

class Node:
    def __init__(self):
        self.children, self.label, self.length = [], None, 0.0


def newick(text):
    """The first tree of ``text`` as nested Nodes."""
    pos = [0]

    def ws():
        while pos[0] < len(text):
            if text[pos[0]] in " \t\r\n":
                pos[0] += 1
            elif text[pos[0]] == "[":
                pos[0] = text.index("]", pos[0]) + 1
            else:
                break

    def name():
        ws()
        if pos[0] < len(text) and text[pos[0]] == "'":
            out = ""
            pos[0] += 1
            while True:
                if text[pos[0]] == "'":
                    if text[pos[0] + 1:pos[0] + 2] == "'":
                        out += "'"
                        pos[0] += 2
                        continue
                    pos[0] += 1
                    return out
                out += text[pos[0]]
                pos[0] += 1
        out = ""
        while pos[0] < len(text) and text[pos[0]] not in "()[],:;' \t\r\n":
            out += text[pos[0]]
            pos[0] += 1
        return out

    def subtree():
        ws()
        nd = Node()
        if text[pos[0]] == "(":
            pos[0] += 1
            nd.children.append(subtree())
            ws()
            while text[pos[0]] == ",":
                pos[0] += 1
                nd.children.append(subtree())
                ws()
            assert text[pos[0]] == ")"
            pos[0] += 1
            name()
        else:
            nd.label = name()
        ws()
        if pos[0] < len(text) and text[pos[0]] == ":":
            pos[0] += 1
            ws()
            j = pos[0]
            while j < len(text) and text[j] in "+-.0123456789eE":
                j += 1
            nd.length = float(text[pos[0]:j])
            pos[0] = j
        return nd

    root = subtree()
    ws()
    assert text[pos[0]] == ";"
    return root


def node_tips(nd):
    return [nd.label] if not nd.children else [s for c in nd.children for s in node_tips(c)]


def node_distances(root):
    """{(tip, tip): path length} of nested Nodes: every tip's chain of ancestors, every pair's first common one."""
    chains = {}

    def walk(nd, chain):
        chain = chain + [(id(nd), nd.length)]
        if not nd.children:
            chains[nd.label] = chain
        for c in nd.children:
            walk(c, chain)

    walk(root, [])
    return _pair_distances(chains)


def array_distances(parent, length, tip_node, tip_label):
    """The same from the arrays of a Tree."""
    chains = {}
    for t, v in enumerate(tip_node):
        chain, v = [], int(v)
        while v >= 0:
            chain.append((v, float(length[v])))
            v = int(parent[v])
        chains[tip_label[t]] = chain[::-1]
    return _pair_distances(chains)


def _pair_distances(chains):
    out = {}
    for a, ca in chains.items():
        for b, cb in chains.items():
            k = 0
            while k < len(ca) and k < len(cb) and ca[k][0] == cb[k][0]:
                k += 1
            out[(a, b)] = sum(x[1] for x in ca[k:]) + sum(x[1] for x in cb[k:])
    return out


def array_depths(parent, length):
    out = []
    for v in range(len(parent)):
        d, u = 0.0, v
        while parent[u] >= 0:
            d += float(length[u])
            u = int(parent[u])
        out.append(d)
    return out


# ---- R/preptrees.R:67-179 over lists --------------------------------------------------------------------------------------------------------------------

def read_table(path):
    """read.table(sep = "\\t", header = T, quote = "", comment.char = ""): (column names, rows of cells: integer, number or string)."""
    def cell(s):
        for f in (int, float):
            try:
                return f(s)
            except ValueError:
                pass
        return s

    with open(path) as fh:
        lines = [ln.rstrip("\n") for ln in fh if ln.strip("\n")]
    return lines[0].split("\t"), [[cell(s) for s in ln.split("\t")] for ln in lines[1:]]


def r_index(n):
    """R's 1:n as a list."""
    n = math.floor(n)
    return list(range(1, n + 1)) if n >= 1 else [1, 0]


def selection(tip_label, pos, fasta_names, fasta_seqs, links_df=None, lr_tophits=None, lr_annotated=None, sr_tophits=None, sr_annotated=None, metadata=None,
              ntop_links=10, frm=None, to=None):
    """Tables are (names, rows).  Returns dict(pos_plot, columns (characters [tips][kept]), warnings, md_names, md_rows)."""
    warn = []
    if links_df is not None:                                           # :67-68
        names, top_hits = links_df[0], [list(r) for r in links_df[1]]
    else:
        def drop_srp(tab, what):                                       # :75-76, :80-81
            if tab is None:
                return None
            idx = [k for k, c in enumerate(tab[0]) if c.lower() == "srp"]
            if len(idx) != 1:
                raise ValueError(what + " file does not contain the srp column!")
            return [c for k, c in enumerate(tab[0]) if k != idx[0]], [[v for k, v in enumerate(r) if k != idx[0]] for r in tab[1]]

        def bind(x, y):
            if x is None:
                return y
            if y is None:
                return x
            assert x[0] == y[0]
            return x[0], x[1] + y[1]

        def dedup(tab, tag):                                           # :84-85
            if tab is None:
                return None
            rows = []
            for r in tab[1]:
                if r not in rows:
                    rows.append(r)
            return tab[0] + ["link"], [r + [tag] for r in rows]

        srl = dedup(bind(drop_srp(sr_tophits, "sr_tophits"), drop_srp(sr_annotated, "sr_annotated_links")), "sr")
        lrl = dedup(bind(lr_tophits, lr_annotated), "lr")
        th = bind(srl, lrl)                                            # :86
        names, top_hits = th if th is not None else ([], [])
    col = {c: [r[k] for r in top_hits] for k, c in enumerate(names)}
    if len(fasta_seqs) and len(fasta_seqs[0]) != len(pos):
        raise ValueError("fasta / pos length mismatch")
    order_idx = []                                                     # :226-233
    for lab in tip_label:
        idx = [k for k, s in enumerate(fasta_names) if s == lab]
        if len(idx) != 1:
            raise ValueError("Sequence names mismatch between provided tree file and fasta file")
        order_idx.append(idx[0])
    fasta = [fasta_seqs[k] for k in order_idx]
    if metadata is not None:                                           # :93-96
        md_id_col = [k for k, c in enumerate(metadata[0]) if c.lower() == "id"]
        if len(md_id_col) != 1:
            raise ValueError("Metadata file must contain an ID column")
    if frm is not None and to is None:                                 # :100-109
        raise ValueError("<to> must also be provided")
    if to is not None and frm is None:
        raise ValueError("<from> must also be provided")
    if frm is not None and to is not None:
        if to < frm:
            raise ValueError("<from> must be less than <to>")
        if frm < 0:
            raise ValueError("<from> must be positive")
        frm, to = round(frm), round(to)
        ntop_links = None
    if ntop_links is not None:                                         # :112-116
        if ntop_links < 0:
            raise ValueError("<ntop_links> must be positive")
        if ntop_links > 10:
            warn.append("Plot may be cluttered due to large <ntop_links> value")
    chosen = []                                                        # :120-130
    if ntop_links is not None and top_hits:
        if links_df is not None:
            chosen += r_index(ntop_links)
        else:
            lr_l = [k + 1 for k, v in enumerate(col["link"]) if v == "lr"]
            if lr_l:
                chosen += [lr_l[k - 1] if 1 <= k <= len(lr_l) else None for k in r_index(ntop_links) if k != 0]
            sr_l = [k + 1 for k, v in enumerate(col["link"]) if v == "sr"]
            if sr_l:
                chosen += [sr_l[k - 1] if 1 <= k <= len(sr_l) else None for k in r_index(ntop_links) if k != 0]
    if frm is not None and to is not None:                             # :132-136
        both = [k + 1 for k, v in enumerate(col.get("pos1", [])) if frm <= v <= to] + [k + 1 for k, v in enumerate(col.get("pos2", [])) if frm <= v <= to]
        chosen = []
        for k in both:
            if k not in chosen:
                chosen.append(k)
    chosen = [k for k in chosen if k is not None and 1 <= k <= len(top_hits)]     # (NA and 0 subscripts give NA / nothing, which sort() drops)
    pos_plot, snp_pos2 = [], []
    if chosen:                                                         # :139-151
        vals = []
        for k in chosen:
            vals += [col["pos1"][k - 1], col["pos2"][k - 1]]
        cand = []
        for v in sorted(vals):
            if v not in cand:
                cand.append(v)
        for v in cand:
            idx = [j for j, q in enumerate(pos) if q == v]
            if len(idx) != 1:
                warn.append("%s not available in the provided fasta file(s)" % (int(v) if float(v).is_integer() else v))
                continue
            snp_pos2.append(idx[0])
            pos_plot.append(v)
    columns = [[row[j] for j in snp_pos2] for row in fasta]
    md_names, md_rows = [], []
    if metadata is not None:                                           # :165-179
        md_id = [str(r[md_id_col[0]]) for r in metadata[1]]
        for lab in tip_label:
            tmp = [k for k, s in enumerate(md_id) if s == lab]
            if not tmp:
                raise ValueError("Entry in tree$tip.label missing in <metadata_df> ids")
            md_rows.append([v for k, v in enumerate(metadata[1][tmp[0]]) if k != md_id_col[0]])
        md_names = [c for k, c in enumerate(metadata[0]) if k != md_id_col[0]]
    return dict(pos_plot=pos_plot, columns=columns, warnings=warn, md_names=md_names, md_rows=md_rows)


# ---- the painter ------------------------------------------------------------------------------------------------------------------------------------------------

def paint_coverage(bars, PW, PH):
    """Coverage sums [PH][PW] (Python ints): every bar adds to every panel pixel its overlap area in 1/256 pixel."""
    cov = [[0] * PW for _ in range(PH)]
    for x0, y0, x1, y1 in bars:
        for py in range(max(0, y0 // 16 - 1), min(PH, y1 // 16 + 2)):
            oy = min(y1, 16 * py + 16) - max(y0, 16 * py)
            if oy <= 0:
                continue
            for px in range(max(0, x0 // 16 - 1), min(PW, x1 // 16 + 2)):
                ox = min(x1, 16 * px + 16) - max(x0, 16 * px)
                if ox > 0:
                    cov[py][px] += ox * oy
    return cov


def paint_panel(bars, PW, PH, fg=0):
    cov = paint_coverage([tuple(int(v) for v in b) for b in bars], PW, PH)
    out = np.zeros((PH, PW, 3), dtype=np.uint8)
    for y in range(PH):
        for x in range(PW):
            ink = min(cov[y][x], 256)
            for k in range(3):
                c = (fg >> (16 - 8 * k)) & 0xFF
                out[y, x, k] = (255 * (256 - ink) + c * ink + 128) >> 8
    return out


def paint_band_line(levels, palette, W):
    """One band's pixel line [W, 3]: per column the overlap-weighted mean of the tips' colours, rounded half up, in integers."""
    N = len(levels)
    out = np.zeros((W, 3), dtype=np.uint8)
    for p in range(W):
        acc = [0, 0, 0]
        total = 0
        for i in range(N):
            ov = min((p + 1) * N, (i + 1) * W) - max(p * N, i * W)
            if ov <= 0:
                continue
            total += ov
            rgb = int(palette[int(levels[i])])
            for k in range(3):
                acc[k] += ov * ((rgb >> (16 - 8 * k)) & 0xFF)
        assert total == N
        for k in range(3):
            out[p, k] = (acc[k] + N // 2) // N
    return out


def paint_band_line_fast(levels, palette, W):
    """paint_band_line for many tips: the same integers, the loop over tips restricted to those that can meet the column."""
    N = len(levels)
    out = np.zeros((W, 3), dtype=np.uint8)
    for p in range(W):
        acc = [0, 0, 0]
        for i in range(max(0, p * N // W - 1), min(N, (p + 1) * N // W + 2)):
            ov = min((p + 1) * N, (i + 1) * W) - max(p * N, i * W)
            if ov <= 0:
                continue
            rgb = int(palette[int(levels[i])])
            for k in range(3):
                acc[k] += ov * ((rgb >> (16 - 8 * k)) & 0xFF)
        for k in range(3):
            out[p, k] = (acc[k] + N // 2) // N
    return out


def paint_canvas(W, H, panel, bars, fg, levels, palette, rects):
    out = np.full((H, W, 3), 255, dtype=np.uint8)
    x, y, w, h = (int(v) for v in panel)
    out[y:y + h, x:x + w] = paint_panel(bars, w, h, fg)
    for r, (bx, by, bw, bh) in enumerate(np.asarray(rects).reshape(-1, 4).tolist()):
        out[by:by + bh, bx:bx + bw] = paint_band_line_fast(levels[r], palette[r], bw)[None, :, :]
    return out
