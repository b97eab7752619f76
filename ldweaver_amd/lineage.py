"""The lineage check for links: does an association hold inside the lineages, or only between them?  ``sequence_clusters`` cuts the
sequences into single-linkage clusters of the Hamming distances (``Engine.seq_clusters``); ``link_lineage_mi`` evaluates the weighted MI of every link
inside each cluster (``Engine.links_stratified``) and appends the summary: a pair of lineage markers has a large MI over the whole sample and none
within any lineage, an epistatic pair keeps its MI within them.  ``link_permutation_test`` gives every link a p-value for its MI from
permutations of one SNP's states among the sequences of each cluster (``Engine.links_permuted``).  All run on the device over the alignment the engine
holds."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

SMALL_MODES = ("drop", "pool")


@dataclass
class SeqClusters:
    """``labels`` int32 [N]: the cluster of every sequence, -1 for a dropped one; ``sizes`` int64 [C]; ``thresh``: neighbours differ in fewer SNP columns
    than this; ``seq_names`` in sequence order."""
    labels: np.ndarray
    sizes: np.ndarray
    thresh: int
    seq_names: list = field(default_factory=list)

    @property
    def n_clusters(self) -> int:
        return int(len(self.sizes))

    def frame(self):
        """An ``ID`` + ``cluster`` frame, one row per sequence: what ``view_tree(metadata_df=)`` takes."""
        import pandas as pd
        return pd.DataFrame({"ID": [str(s) for s in self.seq_names], "cluster": self.labels})


def apply_min_size(labels, min_size: int = 1, small: str = "drop"):
    """(labels int32 [N], sizes int64 [C]) from canonical labels (0 .. n-1 in the order of the clusters' smallest members, -1 allowed): clusters of fewer
    than ``min_size`` members are dropped (label -1) under ``small="drop"`` or pooled into ONE last cluster under ``small="pool"``; the others are
    renumbered 0, 1, ... in the order of their smallest member."""
    if small not in SMALL_MODES:
        raise ValueError(f"small must be one of {SMALL_MODES}, got {small!r}")
    lab = np.asarray(labels, dtype=np.int64)
    n = int(lab.max()) + 1 if len(lab) and lab.max() >= 0 else 0
    size = np.bincount(lab[lab >= 0], minlength=n)
    keep = size >= int(min_size)
    new = np.where(keep, np.cumsum(keep) - 1, -1)
    n_keep = int(keep.sum())
    pooled = small == "pool" and bool((~keep & (size > 0)).any())
    if pooled:
        new[~keep] = n_keep
    out = np.where(lab >= 0, new[np.maximum(lab, 0)] if n else -1, -1).astype(np.int32)
    return out, np.bincount(out[out >= 0], minlength=n_keep + int(pooled)).astype(np.int64)


def _is_missing(x) -> bool:
    return x is None or (isinstance(x, (float, np.floating)) and np.isnan(x)) or type(x).__name__ in ("NAType", "NaTType")


def cluster_labels(clusters, seq_names=None):
    """(labels int32 [N], C) for ``ldw_links_stratified`` from ``clusters``: a ``SeqClusters``; per-sequence levels in sequence order (any array-like of
    length N); or levels matched BY NAME — a pandas Series indexed by sequence name, or a frame with an ``ID`` and a ``cluster`` column (a
    sequence the names do not hold is left out).  Levels are mapped to 0 .. C-1 in the order of their first appearance along the sequences; a missing
    value (None, NaN) maps to -1."""
    if isinstance(clusters, SeqClusters):
        return np.asarray(clusters.labels, dtype=np.int32), clusters.n_clusters
    by_name = None
    if hasattr(clusters, "columns"):         # a frame
        if "ID" not in clusters.columns or "cluster" not in clusters.columns:
            raise ValueError("a frame of clusters needs the columns ID and cluster")
        by_name = dict(zip((str(s) for s in clusters["ID"]), clusters["cluster"].tolist()))
    elif hasattr(clusters, "index") and hasattr(clusters, "tolist"):   # a Series
        by_name = dict(zip((str(s) for s in clusters.index), clusters.tolist()))
    if by_name is not None:
        if seq_names is None:
            raise ValueError("labels matched by name need the sequence names")
        levels = [by_name.get(str(s)) for s in seq_names]
    else:
        levels = np.asarray(clusters).tolist() if not isinstance(clusters, list) else clusters
        if seq_names is not None and len(levels) != len(seq_names):
            raise ValueError(f"{len(levels)} labels for {len(seq_names)} sequences")
    code, out = {}, np.full(len(levels), -1, dtype=np.int32)
    for k, v in enumerate(levels):
        if _is_missing(v):
            continue
        out[k] = code.setdefault(v, len(code))
    return out, len(code)


def lineage_summary(mi, mi_all, poly, neff) -> dict:
    """The columns ``link_lineage_mi`` appends, from the (K, C) matrix ``mi``, ``mi_all`` [K], the flags ``poly`` (K, C) and ``neff`` [C]:
    ``mi_within`` = sum_c neff_c MI_c / sum_c neff_c; ``within_frac`` = mi_within / mi_all (NaN where mi_all <= 0); ``n_poly`` the clusters in which both
    SNPs are polymorphic; ``top_cluster`` the cluster with the largest neff_c MI_c and ``top_share`` its share of the sum (-1 and NaN where the sum is 0)."""
    mi, mi_all, neff = np.asarray(mi, dtype=np.float64), np.asarray(mi_all, dtype=np.float64), np.asarray(neff, dtype=np.float64)
    w = mi * neff[None, :]
    tot = w.sum(axis=1)
    within = tot / neff.sum()
    ok = mi_all > 0
    frac = np.full(len(mi_all), np.nan)
    frac[ok] = within[ok] / mi_all[ok]
    some = tot != 0
    top = np.where(some, np.argmax(w, axis=1) if w.shape[1] else 0, -1).astype(np.int64)
    share = np.full(len(mi_all), np.nan)
    share[some] = w.max(axis=1)[some] / tot[some]
    return dict(mi_within=within, within_frac=frac, n_poly=(np.asarray(poly) == 3).sum(axis=1).astype(np.int64), top_cluster=top, top_share=share)


def permutation_columns(mi_obs, n_ge, null_max, n_perm) -> dict:
    """The columns ``link_permutation_test`` appends: ``mi_all`` the observed MI, ``perm_ge`` the replicates whose MI reaches it, ``perm_p`` =
    (1 + perm_ge) / (1 + n_perm) — the observed arrangement counts as one of the permutations, so no p is 0 —, ``null_max`` the largest replicate MI
    and ``n_perm``."""
    n_perm = int(n_perm)
    if n_perm < 1:
        raise ValueError(f"n_perm must be at least 1, got {n_perm}")
    ge = np.asarray(n_ge, dtype=np.int64)
    if ge.size and (ge.min() < 0 or ge.max() > n_perm):
        raise ValueError("a count of replicates lies outside 0 .. n_perm")
    return dict(mi_all=np.asarray(mi_obs, dtype=np.float64), perm_ge=ge, perm_p=(1.0 + ge) / (1.0 + n_perm),
                null_max=np.asarray(null_max, dtype=np.float64), n_perm=np.full(len(ge), n_perm, dtype=np.int64))


def sequence_clusters(snp_dat=None, *, threshold=0.1, snps=None, min_size: int = 1, small: str = "drop", engine=None, alignment_resident: bool = False):
    """Single-linkage clusters of the sequences: i and j are neighbours iff they differ in fewer than ``thresh`` SNP columns, ``thresh`` =
    ``int(L * threshold)`` — the rule of the Hamming weights — or the absolute ``snps``.  Either may be a list (up to 16 values, served from one Hamming
    GEMM): the result is then a list.  Clusters of fewer than ``min_size`` members are dropped (label -1) or, under ``small="pool"``, pooled into one
    last cluster; the rest are numbered in the order of their smallest member.  Returns a ``SeqClusters`` (labels, sizes, thresh, seq_names; ``.frame()``
    for ``view_tree(metadata_df=)``).  ``engine`` / ``alignment_resident`` as for ``nj_tree``.  Needs a GPU."""
    from .parsimony import _engine_for, _names
    if small not in SMALL_MODES:
        raise ValueError(f"small must be one of {SMALL_MODES}, got {small!r}")
    eng, own = _engine_for(snp_dat, engine, alignment_resident, "sequence_clusters")
    try:
        one = np.ndim(threshold if snps is None else snps) == 0
        th = [int(eng.L * float(t)) for t in np.atleast_1d(threshold)] if snps is None else [int(t) for t in np.atleast_1d(snps)]
        labels, _ = eng.seq_clusters(th)
        names = _names(snp_dat, eng.N)
    finally:
        if own:
            eng.close()
    out = [SeqClusters(*apply_min_size(labels[k], min_size, small), thresh=th[k], seq_names=names) for k in range(len(th))]
    return out[0] if one else out


def link_lineage_mi(links, clusters, snp_dat=None, *, hdw=None, threshold: float = 0.1, engine=None, alignment_resident: bool = False,
                    weights_resident: bool = False, per_cluster: bool = False, out_path=None):
    """``links`` — a frame with ``pos1`` / ``pos2``, or the path of a top-hits file (``read_TopHits``) — with six columns appended, rows and order
    unchanged: ``mi_all``, the weighted MI of the pair over all labelled sequences; ``mi_within``, ``within_frac``, ``n_poly``, ``top_cluster`` and
    ``top_share`` (``lineage_summary``).  ``clusters``: a ``sequence_clusters`` result or any per-sequence labels (``cluster_labels``).  The weights are
    ``hdw``, or the ones the engine holds (``weights_resident``), or the Hamming weights at ``threshold`` as ``estimate_Hamming_distance_weights`` computes
    them; they are the global ones in every cluster.  Positions map to SNPs by ``positions_to_snp_index``.  ``per_cluster=True`` returns (frame, the
    (K, C) matrix of the clusters' MI).  With ``out_path`` the frame is also written as a tab-separated file with a header line, through the native
    table writer where every column is numeric.  ``engine`` / ``alignment_resident`` as for ``nj_tree``.  Needs a GPU."""
    import os
    from .parsimony import _engine_for, _names, _snp_index
    if isinstance(links, (str, bytes, os.PathLike)):
        from .output import read_TopHits
        links = read_TopHits(links)
    df = links.copy()
    a, b = _snp_index(snp_dat, df["pos1"], "link_lineage_mi"), _snp_index(snp_dat, df["pos2"], "link_lineage_mi")
    if weights_resident and (engine is None or hdw is not None):
        raise ValueError("weights_resident=True needs the engine that holds the weights, and no hdw")
    eng, own = _engine_for(snp_dat, engine, alignment_resident, "link_lineage_mi")
    try:
        labels, C = cluster_labels(clusters, _names(snp_dat, eng.N))
        if len(labels) != eng.N:
            raise ValueError(f"{len(labels)} cluster labels for {eng.N} sequences")
        if C < 1:
            raise ValueError("link_lineage_mi: no sequence has a cluster")
        if not weights_resident:
            eng.set_weights(eng.hamming_weights(int(eng.L * float(threshold))) if hdw is None else hdw)
        if len(df):
            res = eng.links_stratified(a, b, labels, C)
        else:
            res = dict(mi=np.zeros((0, C)), mi_all=np.zeros(0), poly=np.zeros((0, C), dtype=np.uint8), neff=np.ones(C))
    finally:
        if own:
            eng.close()
    df["mi_all"] = res["mi_all"]
    for name, col in lineage_summary(res["mi"], res["mi_all"], res["poly"], res["neff"]).items():
        df[name] = col
    if out_path is not None:
        _write_frame(df, out_path)
    return (df, res["mi"]) if per_cluster else df


def link_permutation_test(links, clusters=None, snp_dat=None, *, n_perm: int = 1000, seed: int = 0, hdw=None, threshold: float = 0.1, engine=None,
                          alignment_resident: bool = False, return_null: bool = False, out_path=None):
    """``links`` — as ``link_lineage_mi`` takes them — with five columns appended, rows and order unchanged (``permutation_columns``): ``mi_all``,
    ``perm_ge``, ``perm_p``, ``null_max`` and ``n_perm``.  Each of the ``n_perm`` replicates permutes the second SNP's states among the sequences of
    every cluster and re-evaluates the weighted MI over all labelled sequences, so population structure that the clusters capture is in the null: a
    pair of lineage markers keeps its table in every replicate (p = 1), a pair coupled inside the lineages gets a small p.  ``clusters``: as for
    ``link_lineage_mi``; None means one cluster, the unrestricted test.  The weights are ``hdw``, or the Hamming weights at ``threshold``; they stay
    with the sequences.  A replicate is a function of (clusters, ``seed``, its number) alone.  ``return_null=True`` returns (frame, the (K, n_perm)
    matrix of the replicates' MI).  ``out_path``, ``engine`` / ``alignment_resident`` as for ``link_lineage_mi``.  Needs a GPU."""
    import os
    from .parsimony import _engine_for, _names, _snp_index
    n_perm = int(n_perm)
    if not 1 <= n_perm <= 1 << 24:
        raise ValueError(f"n_perm must lie in 1 .. 2^24, got {n_perm}")
    if isinstance(links, (str, bytes, os.PathLike)):
        from .output import read_TopHits
        links = read_TopHits(links)
    df = links.copy()
    a, b = _snp_index(snp_dat, df["pos1"], "link_permutation_test"), _snp_index(snp_dat, df["pos2"], "link_permutation_test")
    eng, own = _engine_for(snp_dat, engine, alignment_resident, "link_permutation_test")
    try:
        if clusters is None:
            labels, C = np.zeros(eng.N, dtype=np.int32), 1
        else:
            labels, C = cluster_labels(clusters, _names(snp_dat, eng.N))
        if len(labels) != eng.N:
            raise ValueError(f"{len(labels)} cluster labels for {eng.N} sequences")
        if C < 1:
            raise ValueError("link_permutation_test: no sequence has a cluster")
        eng.set_weights(eng.hamming_weights(int(eng.L * float(threshold))) if hdw is None else hdw)
        if len(df):
            res = eng.links_permuted(a, b, labels, n_perm, seed=seed, C=C, want_null=return_null)
        else:
            res = dict(mi_obs=np.zeros(0), n_ge=np.zeros(0, dtype=np.int32), null_max=np.zeros(0), null=np.zeros((0, n_perm)))
    finally:
        if own:
            eng.close()
    for name, col in permutation_columns(res["mi_obs"], res["n_ge"], res["null_max"], n_perm).items():
        df[name] = col
    if out_path is not None:
        _write_frame(df, out_path)
    return (df, res["null"]) if return_null else df


def _write_frame(df, path):
    """Header line, then the rows: by the native table writer where every column is numeric, else by pandas."""
    if all(df[c].dtype.kind in "iubf" for c in df.columns):
        from .engine import write_table_tsv
        with open(path, "w") as fh:
            fh.write("\t".join(str(c) for c in df.columns) + "\n")
        write_table_tsv(str(path), [df[c].to_numpy() for c in df.columns], append=True)
    else:
        df.to_csv(path, sep="\t", index=False)
