"""What the network tests compare against: a literal pandas restatement of R/createNetworkPlot.R:36-118 (create_network's edge list) and
:169-290 (create_network_for_gene) with LITERAL matching, and a naive per-pixel numpy painter of the capsule rule (include/ldweaver_amd.h 12).
Written against the R text, line by line, with data frames where the product walks lists."""
import csv

import numpy as np
import pandas as pd

FRAME_COLS = ["pos1", "pos2", "pos1_ann", "pos2_ann", "MI", "links", "ARACNE"]


def _tok(x, separator):                                      # unlist(strsplit(x, separator))[1], literal
    return x.split(separator)[0]


def _ddply(p1a, p2a):
    """plyr::ddply(df, .(p1a, p2a), nrow): one row per distinct pair, sorted by p1a, then p2a."""
    d = pd.DataFrame({"p1a": p1a, "p2a": p2a})
    g = d.groupby(["p1a", "p2a"], sort=True).size().reset_index(name="V1")
    return g


def edges(tophits, separator=":", max_plot_nodes=None, min_links_to_include=2):
    n = len(tophits)
    if max_plot_nodes is None:                               # :40-45
        avail_links = n
        max_plot_nodes = n
    else:
        avail_links = max_plot_nodes
    c50 = True
    while c50:                                               # :49-65
        k = min(avail_links, n)                              # (R reads NA past the end: a group its loop filter drops again)
        p1a = [_tok(x, separator) for x in tophits["pos1_ann"].iloc[:k]]
        p2a = [_tok(x, separator) for x in tophits["pos2_ann"].iloc[:k]]
        df = pd.DataFrame({"p1a": p1a, "p2a": p2a, "w": tophits["MI"].to_numpy(dtype=float)[:k]})
        df_uq = _ddply(p1a, p2a)
        if len(df_uq) >= max_plot_nodes:
            c50 = False
        avail_links += 1
        if avail_links > n:
            c50 = False
    df_uq = df_uq[df_uq["V1"] >= min_links_to_include].reset_index(drop=True)      # :67
    df_uq["w"] = [df["w"][(df["p1a"] == a) & (df["p2a"] == b)].max() for a, b in zip(df_uq["p1a"], df_uq["p2a"])]      # :70-72
    swp_lr = df_uq["p1a"].isin(df_uq["p2a"]).to_numpy()                              # :75-80
    if swp_lr.any():
        tmp = df_uq.loc[swp_lr, "p1a"].to_numpy()
        df_uq.loc[swp_lr, "p1a"] = df_uq.loc[swp_lr, "p2a"].to_numpy()
        df_uq.loc[swp_lr, "p2a"] = tmp
    swp_rl = df_uq["p2a"].isin(df_uq["p1a"]).to_numpy()                              # :82-87
    if swp_rl.any():
        tmp = df_uq.loc[swp_rl, "p1a"].to_numpy()
        df_uq.loc[swp_rl, "p1a"] = df_uq.loc[swp_rl, "p2a"].to_numpy()
        df_uq.loc[swp_rl, "p2a"] = tmp
    pst1 = (df_uq["p1a"] + " " + df_uq["p2a"]).tolist()                              # :91-92
    pst2 = (df_uq["p2a"] + " " + df_uq["p1a"]).tolist()
    for i in [i for i, x in enumerate(pst1) if x in pst2]:                           # :94-106
        mrg = pst1[i].split(" ")
        if len(mrg) < 2:
            continue
        l1 = np.nonzero(((df_uq["p1a"] == mrg[0]) & (df_uq["p2a"] == mrg[1])).to_numpy())[0]
        l2 = np.nonzero(((df_uq["p1a"] == mrg[1]) & (df_uq["p2a"] == mrg[0])).to_numpy())[0]
        if len(l1) == 1 and len(l2) == 1:
            a, b = df_uq.index[l1[0]], df_uq.index[l2[0]]
            v, w = df_uq.loc[[a, b], "V1"].sum(), df_uq.loc[[a, b], "w"].max()
            df_uq.loc[a, "V1"] = v
            df_uq.loc[a, "w"] = w
            df_uq = df_uq.drop(index=b).reset_index(drop=True)
    kps = (df_uq["p1a"] != df_uq["p2a"]).to_numpy()                                   # :109-117
    if not kps.any():
        raise ValueError("Everything is a loop!")
    s_weights = df_uq["w"].to_numpy(dtype=float)[kps]
    return pd.DataFrame({"p1": df_uq["p1a"].to_numpy()[kps], "p2": df_uq["p2a"].to_numpy()[kps], "Num_Links": df_uq["V1"].to_numpy(dtype=np.int64)[kps],
                         "weights": s_weights / s_weights.max()})                     # :118


def read_annotated(path):
    """read.table(sep = "\\t", quote = "", header = T) with the string columns kept as text."""
    return pd.read_csv(path, sep="\t", header=0, quoting=csv.QUOTE_NONE, dtype={"pos1_ann": str, "pos2_ann": str, "links": str}, keep_default_na=False,
                       na_values={c: ["NA", "NaN", "nan"] for c in ("pos1", "pos2", "len", "ARACNE", "MI")}, float_precision="round_trip")


def grep_rows(tab, needle):
    """sort(unique(c(grep(needle, pos1_ann, fixed = T), grep(needle, pos2_ann, fixed = T)))): row numbers, ascending."""
    hit = tab["pos1_ann"].str.contains(needle, regex=False) | tab["pos2_ann"].str.contains(needle, regex=False)
    return np.nonzero(hit.to_numpy())[0]


def _pick(tab, idx):
    t = tab.iloc[idx]
    return pd.DataFrame({c: t[c].to_numpy() for c in FRAME_COLS}, columns=FRAME_COLS).astype({"pos1": float, "pos2": float, "MI": float, "ARACNE": float})


def _drop(df, drop_syXsy, drop_indirect):
    if drop_syXsy:
        df = df[df["links"] != "syXsy"]
    if drop_indirect:
        df = df[df["ARACNE"] == 1]
    return df.reset_index(drop=True)


def for_gene(gene_name, sr=None, lr=None, drop_syXsy=True, drop_indirect=True, level=1, separator=":", min_links_to_include=3):
    tabs = [read_annotated(p) for p in (sr, lr) if p is not None]
    parts = [_pick(t, grep_rows(t, gene_name)) for t in tabs]                        # :177-209
    df = _drop(pd.concat(parts, ignore_index=True), drop_syXsy, drop_indirect)        # :211-216
    if level == 2 and len(df):                                                        # :219-281
        p1a = [_tok(x, separator) for x in df["pos1_ann"]]
        p2a = [_tok(x, separator) for x in df["pos2_ann"]]
        df_uq = _ddply(p1a, p2a)
        df_uq = df_uq[df_uq["V1"] >= min_links_to_include]
        genes = list(pd.unique(np.asarray(df_uq["p1a"].tolist() + df_uq["p2a"].tolist(), dtype=object)))
        which = [i for i, g in enumerate(genes) if g == gene_name]
        genes = [g for i, g in enumerate(genes) if i not in which] if which else []    # genes[-integer(0)] is empty
        for gene in genes:
            df = pd.concat([df] + [_pick(t, grep_rows(t, gene)) for t in tabs], ignore_index=True)
        df = _drop(df, drop_syXsy, drop_indirect)
    df = df[~df.duplicated()].reset_index(drop=True)                                  # :284-285
    for c in ("pos1", "pos2", "ARACNE"):
        v = df[c].to_numpy(dtype=float)
        if len(v) and np.all(np.isfinite(v)) and np.all(v == np.floor(v)):
            df[c] = v.astype(np.int64)
    return df


def paint(caps, W, H):
    """The capsule rule, pixel by pixel: caps = iterable of (x0, y0, x1, y1, w, rgb, alpha) in draw order; uint8 [H, W, 3]."""
    img = np.full((H, W, 3), 255, dtype=np.int64)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.int64)
    for x0, y0, x1, y1, w, rgb, a in caps:
        x0, y0, x1, y1, w, rgb, a = (int(v) for v in (x0, y0, x1, y1, w, rgb, a))
        px, py, dx, dy = xs - x0, ys - y0, x1 - x0, y1 - y0
        dd, t = dx * dx + dy * dy, px * dx + py * dy
        d0 = 4 * (px * px + py * py) <= w * w
        d1 = 4 * ((px - dx) ** 2 + (py - dy) ** 2) <= w * w
        mid = 4 * (px * dy - py * dx) ** 2 <= w * w * dd
        cov = np.where(t <= 0, d0, np.where(t >= dd, d1, mid))
        col = np.array([rgb >> 16 & 255, rgb >> 8 & 255, rgb & 255], dtype=np.int64)
        img[cov] = (img[cov] * (255 - a) + col * a + 127) // 255
    return img.astype(np.uint8)
