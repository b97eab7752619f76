"""Restatements of estimate_variation_in_CDS (R/estimateCDSDiversity.R:27-123), perform_clustering (:127-148) and painter (:151-210) for the
tests of ldweaver_amd.cds: a LITERAL port, statement by statement with 1-based indices, region_mat and R's half-even round(), and a
vectorised numpy twin for large inputs.  Where R stops with an error the literal port raises RStop; ``painter_contract`` turns that into
the behaviour the project documents."""
from __future__ import annotations

import math

import numpy as np

ALPHA = ("A", "C", "G", "T", "*")
QUIRK_REFERENCE, QUIRK_INTENDED = 0, 1


class RStop(Exception):
    """An R error of the reference; ``paint`` is the paint as it stood, ``kind`` says which statement stopped."""
    def __init__(self, kind, paint):
        super().__init__(kind)
        self.kind, self.paint = kind, paint


def r_round(x: float) -> int:
    """R's round(x) for the halves painter meets: IEC 60559, a half goes to the even neighbour."""
    f = math.floor(x)
    d = x - f
    if d > 0.5 or (d == 0.5 and f % 2 == 1):
        return int(f) + 1
    return int(f)


# ---------------------------------------------------------------------------------------------------------------------------------------
# literal port
# ---------------------------------------------------------------------------------------------------------------------------------------
def acgtn2num_literal(reference, ref):
    """src/ACGTN2num_parallel.cpp:10-43: zero the reference row of each column; case-sensitive, N and '-' -> row 5."""
    for c, ch in enumerate(ref):
        if ch == "A":
            reference[0, c] = 0
        elif ch == "C":
            reference[1, c] = 0
        elif ch == "G":
            reference[2, c] = 0
        elif ch == "T":
            reference[3, c] = 0
        elif ch == "N" or ch == "-":
            reference[4, c] = 0


def variation_literal(POS, variation, ref_seq: bytes, starts, ends):
    """R/estimateCDSDiversity.R:54-105 (gff branch).  Returns var_estimate (None = NA), snp_var, alt, ref."""
    nsnp = len(POS)
    ref = [chr(ref_seq[int(p) - 1]) for p in POS]
    widths = [int(e) - int(s) + 1 for s, e in zip(starts, ends)]
    ncds = len(starts)
    var_estimate = [None] * ncds
    reference = np.ones((5, nsnp))
    acgtn2num_literal(reference, ref)
    variation_wo_ref = np.asarray(variation, dtype=np.float64) * reference
    alt = [",".join(ALPHA[x] for x in range(5) if variation_wo_ref[x, s] > 0) for s in range(nsnp)]
    snp_var = [float(sum(variation_wo_ref[:, s])) for s in range(nsnp)]
    for cds in range(ncds):
        pos_idx = [i for i in range(nsnp) if starts[cds] <= POS[i] <= ends[cds]]     # %between%: inclusive
        if len(pos_idx) > 0:
            var_estimate[cds] = sum(snp_var[i] for i in pos_idx) / widths[cds]
    return var_estimate, snp_var, alt, ref


def relabel_literal(cluster):
    """perform_clustering's relabelling (:129-137) of a kmeans cluster vector (ids 1..k); R's order(decreasing = T) is stable."""
    ids = sorted(set(cluster))
    counts = [sum(1 for c in cluster if c == i) for i in ids]
    km_ord = [ids[j] for j in sorted(range(len(ids)), key=lambda j: -counts[j])]
    km_clst_ord = list(cluster)
    for i in range(1, len(km_ord) + 1):
        if i != km_ord[i - 1]:
            for q, c in enumerate(cluster):
                if c == km_ord[i - 1]:
                    km_clst_ord[q] = i
    return km_clst_ord


def perform_clustering_literal(var_estimate, nclust, kmeans_cluster):
    """``kmeans_cluster(x, k)`` stands for km$cluster (ids 1..k)."""
    cl = kmeans_cluster(var_estimate, nclust)
    km_clst_ord = relabel_literal(list(cl))
    cutoff = max(v for v, c in zip(var_estimate, km_clst_ord) if c == 1)
    return km_clst_ord, cutoff


def painter_literal(POS, km_clst_ord, cds_start, cds_end, quirk=QUIRK_REFERENCE):
    n = len(POS)
    paint = [0] * n
    for i in range(1, len(set(km_clst_ord)) + 1):
        c1 = [(cds_start[j], cds_end[j]) for j in range(len(km_clst_ord)) if km_clst_ord[j] == i]
        for j in range(len(c1)):
            for q in range(n):
                if c1[j][0] < POS[q] and POS[q] < c1[j][1]:
                    paint[q] = i
    if n == 1:
        raise RStop("2:1 iterates downwards: paint[2] is NA", list(paint))
    begin = 1
    prev_val = paint[0]
    region_mat = []
    update = False
    for i in range(2, n + 1):
        if paint[i - 1] != prev_val:
            end = i - 1
            region_mat.append([prev_val, begin, end])
            begin = i
            prev_val = paint[i - 1]
            update = True
        if i == n:
            if update and quirk == QUIRK_REFERENCE:
                break
            region_mat.append([prev_val, begin, i])
        update = False
    if region_mat[0][0] == 0:
        if len(region_mat) < 2:
            raise RStop("region_mat[1, 2]: subscript out of bounds", list(paint))
        r = region_mat[0]
        for q in range(r[1], r[2] + 1):
            paint[q - 1] = region_mat[1][0]
        region_mat[0][0] = region_mat[1][0]
    if region_mat[-1][0] == 0:
        if len(region_mat) < 2:
            raise RStop("region_mat[1, 0]: subscript out of bounds", list(paint))
        r = region_mat[-1]
        for q in range(r[1], r[2] + 1):
            paint[q - 1] = region_mat[-2][0]
        region_mat[-1][0] = region_mat[-2][0]
    rm0s = [c for c in range(len(region_mat)) if region_mat[c][0] == 0]
    if len(rm0s) == 0:
        raise RStop("1:length(rm0s) iterates over c(1, 0): region_mat[, NA]", list(paint))
    for c in rm0s:
        r = region_mat[c]
        if r[1] == r[2]:
            paint[r[1] - 1] = region_mat[c - 1][0]
        else:
            ss = r_round((r[2] - r[1]) / 2)
            for q in range(r[1], r[1] + ss + 1):
                paint[q - 1] = region_mat[c - 1][0]
            for q in range(r[1] + ss + 1, r[2] + 1):
                paint[q - 1] = region_mat[c + 1][0]
    return paint


def painter_contract(POS, km_clst_ord, cds_start, cds_end, quirk=QUIRK_REFERENCE):
    """The literal painter where R stops: the paint as it stands for L = 1 and for no interior 0 run; ValueError when no recorded run is
    painted (every SNP 0, or only the unrecorded last one)."""
    try:
        return painter_literal(POS, km_clst_ord, cds_start, cds_end, quirk)
    except RStop as e:
        if "subscript out of bounds" in e.kind or not any(e.paint):
            raise ValueError("no SNP lies strictly inside a kept CDS") from None
        return e.paint


def estimate_literal(POS, variation, ref_seq: bytes, starts, ends, nclust, kmeans_cluster, quirk=QUIRK_REFERENCE):
    var_estimate, snp_var, alt, ref = variation_literal(POS, variation, ref_seq, starts, ends)
    cds_idx = [v is not None for v in var_estimate]
    ve = [v for v, k in zip(var_estimate, cds_idx) if k]
    cs = [s for s, k in zip(starts, cds_idx) if k]
    ce = [e for e, k in zip(ends, cds_idx) if k]
    km_clst_ord, cutoff = perform_clustering_literal(ve, nclust, kmeans_cluster)
    paint = painter_contract(list(POS), km_clst_ord, cs, ce, quirk)
    return dict(var_all=np.array([np.nan if v is None else v for v in var_estimate], dtype=np.float64), var_estimate=np.array(ve, dtype=np.float64),
                cds_start=np.array(cs, dtype=np.int64), cds_end=np.array(ce, dtype=np.int64), km_clst_ord=np.array(km_clst_ord, dtype=np.int32),
                cutoff=cutoff, paint=np.array(paint, dtype=np.int32), alt=alt, ref=ref, snp_var=np.array(snp_var, dtype=np.int64))


# ---------------------------------------------------------------------------------------------------------------------------------------
# vectorised twin
# ---------------------------------------------------------------------------------------------------------------------------------------
_ROW = np.full(256, -1, dtype=np.int64)
for _c, _r in zip("ACGTN-", (0, 1, 2, 3, 4, 4)):
    _ROW[ord(_c)] = _r


def variation_vec(POS, counts, ref_seq, starts, ends):
    """(var [ncds] with NaN, snp_var int64 [L], alt_mask uint8 [L], ref uint8 [L])."""
    POS = np.asarray(POS, dtype=np.int64)
    ref = np.frombuffer(bytes(ref_seq), dtype=np.uint8) if isinstance(ref_seq, (bytes, bytearray)) else np.asarray(ref_seq, dtype=np.uint8)
    refc = ref[POS - 1]
    row = _ROW[refc]
    masked = np.asarray(counts, dtype=np.int64).copy()
    has = row >= 0
    masked[row[has], np.flatnonzero(has)] = 0
    snp_var = masked.sum(axis=0)
    alt = ((masked > 0) * (1 << np.arange(5))[:, None]).sum(axis=0).astype(np.uint8)
    order = np.argsort(POS, kind="stable")
    sp = POS[order]
    P = np.concatenate([[0], np.cumsum(snp_var[order])])
    st, en = np.asarray(starts, dtype=np.int64), np.asarray(ends, dtype=np.int64)
    lo, hi = np.searchsorted(sp, st, "left"), np.searchsorted(sp, en, "right")
    ok = (en >= st) & (hi > lo)
    var = np.full(len(st), np.nan)
    var[ok] = (P[hi[ok]] - P[lo[ok]]).astype(np.float64) / (en[ok] - st[ok] + 1).astype(np.float64)
    return var, snp_var, alt, refc


def paint_vec(POS, cds_start, cds_end, labels, quirk=QUIRK_REFERENCE):
    """(paint int32 [L], SNPs left at 0); ValueError as painter_contract."""
    POS = np.asarray(POS, dtype=np.int64)
    n = len(POS)
    order = np.argsort(POS, kind="stable")
    sp = POS[order]
    st, en = np.asarray(cds_start, dtype=np.int64), np.asarray(cds_end, dtype=np.int64)
    lab = np.asarray(labels, dtype=np.int32)
    lo, hi = np.searchsorted(sp, st, "right"), np.searchsorted(sp, en, "left")
    cnt = np.maximum(hi - lo, 0)
    ps = np.zeros(n, dtype=np.int32)
    if cnt.sum() > 0:
        owner = np.repeat(np.arange(len(st)), cnt)
        k = lo[owner] + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        np.maximum.at(ps, k, lab[owner])
    p = np.empty(n, dtype=np.int32)
    p[order] = ps
    change = np.r_[True, p[1:] != p[:-1]]
    begins = np.flatnonzero(change)
    ends_ = np.r_[begins[1:] - 1, n - 1]
    m = len(begins)
    if quirk == QUIRK_REFERENCE and m >= 2 and begins[-1] == n - 1:
        m -= 1
    vals = p[begins[:m]].copy()
    if not np.any(vals != 0):
        raise ValueError("no SNP lies strictly inside a kept CDS")
    if vals[0] == 0:
        vals[0] = vals[1]
    if vals[m - 1] == 0:
        vals[m - 1] = vals[m - 2]
    out = p.copy()
    rid = np.cumsum(change) - 1
    rec = np.flatnonzero(rid < m)
    out[rec] = vals[rid[rec]]
    z = rec[vals[rid[rec]] == 0]
    if len(z):
        r = rid[z]
        b, e = begins[r], ends_[r]
        ss = np.round((e - b) / 2).astype(np.int64)
        out[z] = np.where(z <= b + ss, vals[r - 1], vals[r + 1])
    return out, int((out == 0).sum())


def alt_strings(mask):
    return [",".join(ALPHA[x] for x in range(5) if (int(m) >> x) & 1) for m in mask]


def clusters_by_mean(labels, x):
    """km$cluster as a kmeans object might number it: ids 1..k in ascending order of the cluster's values."""
    labels = np.asarray(labels)
    x = np.asarray(x)
    ks = sorted(set(labels.tolist()), key=lambda l: x[labels == l].min())
    rank = {l: i + 1 for i, l in enumerate(ks)}
    return [rank[l] for l in labels.tolist()]
