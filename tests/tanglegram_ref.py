"""What the tanglegram tests compare against: an O(n^3) complete linkage on the full distance matrix (the tie rule of DESIGN.md 24), a pandas
transliteration of R/createTanglegram.R:35-276 with LITERAL matching, and a naive numpy painter of the render rule (include/ldweaver_amd.h 12):
the capsules by ``network_ref.paint``, then the rectangles in list order."""
import numpy as np
import pandas as pd

import network_ref as NR


def cutree_labels(cluster_of_row):
    """cutree's numbering: 1, 2, ... in order of first appearance by row."""
    first = {}
    return np.asarray([first.setdefault(c, len(first) + 1) for c in cluster_of_row], dtype=np.int64)


def brute_complete_linkage(pos, k):
    """hclust(dist(pos), "complete") cut at k, on the n x n matrix: the distance of two clusters is the largest distance between their members; the
    closest pair is merged.  Tie rule: the points are ranked by (position, row); a cluster is named by its smallest rank; among pairs of equal
    distance the pair with the smallest (left name, right name) is merged."""
    v = np.asarray(pos, dtype=np.float64)
    n = len(v)
    rank = np.empty(n, dtype=np.int64)
    rank[np.argsort(v, kind="stable")] = np.arange(n)
    d = np.abs(v[:, None] - v[None, :])
    clusters = {int(rank[i]): [i] for i in range(n)}
    while len(clusters) > k:
        best = None
        names = sorted(clusters)
        for ia, a in enumerate(names):
            for b in names[ia + 1:]:
                dist = max(d[i, j] for i in clusters[a] for j in clusters[b])
                if best is None or (dist, a, b) < best:
                    best = (dist, a, b)
        _, a, b = best
        clusters[a] += clusters.pop(b)
    of_row = np.zeros(n, dtype=np.int64)
    for name, rows in clusters.items():
        of_row[rows] = name
    return cutree_labels(of_row.tolist())


def _grep(needle, column):
    """grep(needle, column, fixed = TRUE): 0-based row numbers."""
    return [i for i, s in enumerate(column) if isinstance(s, str) and needle in s]


def reference(tophits, break_segments, links_type, cds=None, gff=None, cutree=brute_complete_linkage):
    """R/createTanglegram.R:35-276, line by line.  ``cds``: a frame locus_tag / start / end (the one feature table our record has, with its own
    coordinates); ``gff``: a frame attributes / start / end.  The gff branch tests every name for "not found" as the gbk branch does (the reference's test
    sits outside the loop).  Rows without a region name are left out first.  Returns one dict per clustidx: chr, ann, links (None where nothing is left)."""
    tophits = tophits.reset_index(drop=True).copy()
    tophits["dummy_chrom"] = cutree(tophits["pos1"].to_numpy(dtype=float), break_segments)                       # :35
    mins = [tophits["pos1"][tophits["dummy_chrom"] == x].min() for x in range(1, break_segments + 1)]
    clst_brk_ord = list(np.argsort(np.asarray(mins, dtype=float), kind="stable") + 1)                            # :38
    dc_tmp = tophits["dummy_chrom"].to_numpy().copy()                                                            # :39
    change = False
    for i in range(1, break_segments + 1):                                                                       # :41-48
        if i == clst_brk_ord[i - 1]:
            continue
        dc_tmp[(tophits["dummy_chrom"] == i).to_numpy()] = clst_brk_ord[i - 1]
        change = True
    if change:
        tophits["dummy_chrom"] = dc_tmp
    out = []
    for clustidx in range(1, break_segments + 1):                                                                # :59
        t = tophits[tophits["dummy_chrom"] == clustidx]
        ok = [isinstance(a, str) and isinstance(b, str) and a != "" and b != "" for a, b in zip(t["pos1_genreg"], t["pos2_genreg"])]
        t = t[np.asarray(ok, dtype=bool)]
        if links_type == "SR":                                                                                   # :61-71
            df = pd.DataFrame({"p1a": t["pos1_genreg"].tolist(), "p2a": t["pos2_genreg"].tolist(), "w": t["srp"].to_numpy(dtype=float)})
        elif links_type == "LR":
            df = pd.DataFrame({"p1a": t["pos1_genreg"].tolist(), "p2a": t["pos2_genreg"].tolist(), "w": t["MI"].to_numpy(dtype=float)})
        else:
            raise ValueError("Links type must be SR or LR")
        df_uq = NR._ddply(df["p1a"].tolist(), df["p2a"].tolist())                                                # :74
        df_uq["w"] = [df["w"][(df["p1a"] == a) & (df["p2a"] == b)].max() for a, b in zip(df_uq["p1a"], df_uq["p2a"])]   # :76-80
        all_locs = list(pd.unique(np.asarray(df_uq["p1a"].tolist() + df_uq["p2a"].tolist(), dtype=object)))      # :82

        def locate(locs):
            lse, notfound = [], []
            for name in locs:                                                                                    # :89-137 / :142-158
                if cds is not None:
                    idx, tab = _grep(name, cds["locus_tag"].tolist()), cds
                else:
                    idx, tab = _grep(name.replace("GENE_", ""), gff["attributes"].tolist()), gff
                if idx:
                    lse.append((int(pd.unique(tab["start"].to_numpy()[idx])[0]), int(pd.unique(tab["end"].to_numpy()[idx])[0])))
                else:
                    lse.append((None, None))
                    notfound.append(name)
            return lse, notfound

        loc_strt_end, all_locs_notfound = locate(all_locs)
        if all_locs_notfound:                                                                                    # :164-244
            prune_rows = []
            for nf in all_locs_notfound:
                prune_rows += _grep(nf, df_uq["p1a"].tolist()) + _grep(nf, df_uq["p2a"].tolist())
            df_uq = df_uq.drop(index=sorted(set(prune_rows))).reset_index(drop=True)
            all_locs = list(pd.unique(np.asarray(df_uq["p1a"].tolist() + df_uq["p2a"].tolist(), dtype=object)))
            loc_strt_end, _ = locate(all_locs)
        if not len(df_uq):
            out.append(dict(segment=clustidx, chr=None, ann=None, links=None, all_locs=[]))
            continue
        st, en = [a for a, _ in loc_strt_end], [b for _, b in loc_strt_end]
        chr_file = pd.DataFrame({"V1": ["p", "q"], "V2": np.asarray([min(st) - 1000] * 2, dtype=np.int64), "V3": np.asarray([max(en) + 1000] * 2, dtype=np.int64)})   # :264-266
        ann_file = pd.DataFrame({"V1": ["p_" + s for s in all_locs] + ["q_" + s for s in all_locs], "V2": ["p"] * len(all_locs) + ["q"] * len(all_locs),
                                 "V3": np.asarray(st + st, dtype=np.int64), "V4": np.asarray(en + en, dtype=np.int64)})                                             # :269-272
        link_data = pd.DataFrame({"V1": ["p_" + s for s in df_uq["p1a"]], "V2": np.ones(len(df_uq), dtype=np.int64), "V3": ["q_" + s for s in df_uq["p2a"]],
                                  "V4": np.ones(len(df_uq), dtype=np.int64), "w": df_uq["w"].to_numpy(dtype=float)})                                                 # :275-276
        out.append(dict(segment=clustidx, chr=chr_file, ann=ann_file, links=link_data, all_locs=all_locs))
    return out


def paint_marks(caps, rects, W, H):
    """The render rule: the capsules over white (network_ref.paint), then every rectangle (x0, y0, x1, y1, rgb), half-open and clipped to the canvas,
    opaque in list order."""
    img = NR.paint([tuple(int(v) for v in c) for c in caps], W, H)
    for x0, y0, x1, y1, rgb in rects:
        x0, y0, x1, y1, rgb = (int(v) for v in (x0, y0, x1, y1, rgb))
        xa, xb, ya, yb = max(x0, 0), min(x1, W), max(y0, 0), min(y1, H)
        if xb > xa and yb > ya:
            img[ya:yb, xa:xb] = (rgb >> 16 & 255, rgb >> 8 & 255, rgb & 255)
    return img
