"""The gene-by-gene MI map (include/ldweaver_amd.h 24): a segment x segment matrix over EVERY SNP pair of an alignment — the values the pass
computes and drops — where "segment" is any labelling of the SNPs: the CDSs of an annotation, equal stretches of the genome, or the caller's own.  Per
cell: the pairs, the pairs at or above a threshold, the exact sum of the values in 40-bit fixed point, the largest value and the SNP pair that carries it.
The integers are taken on the device (``Engine.mi_segment_map``, ``Engine.mi_segment_best``); everything in ``GeneMap`` is a pure host function of them."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import pandas as pd

from . import _lib as L
from .background import CLS_MASK, FRAC, WHICH, apc_weights

__all__ = ["segments_from_features", "segments_from_annotation", "segments_equal", "gene_map", "GeneMap"]

LO_BITS = 24                      # bits of q in the low word of a cell's sum (csrc/ldw_segmap.h SEGMAP_LO_BITS)
MAX_SEGMENTS = 8192
NO_PAIR = np.uint64(0xFFFFFFFFFFFFFFFF)
BY = ("nge", "max", "mean")
NAMES = ("n", "nge", "sum_lo", "sum_hi", "max", "mean", "frac", "exact_sum")


def segments_from_features(pos, starts, ends) -> np.ndarray:
    """seg (L,) int32: per SNP the smallest feature index j with starts[j] <= pos <= ends[j] (1-based, inclusive), else -1.  The features may overlap and
    come in any order.  The positions are sorted once and every feature, last index first, writes its index over the stretch of sorted positions it holds:
    the work is (features + L) log L plus the positions covered, never L x features."""
    pos = np.asarray(pos, dtype=np.int64).ravel()
    st, en = np.asarray(starts, dtype=np.int64).ravel(), np.asarray(ends, dtype=np.int64).ravel()
    if st.shape != en.shape:
        raise ValueError("starts and ends differ in length")
    order = np.argsort(pos, kind="stable")
    spos = pos[order]
    lo, hi = np.searchsorted(spos, st, side="left"), np.searchsorted(spos, en, side="right")
    seg_sorted = np.full(len(pos), -1, dtype=np.int32)
    for j in range(len(st) - 1, -1, -1):
        if hi[j] > lo[j]:
            seg_sorted[lo[j]:hi[j]] = j
    seg = np.empty(len(pos), dtype=np.int32)
    seg[order] = seg_sorted
    return seg


def segments_from_annotation(snp_dat, gff=None, gbk=None, feature: str = "CDS"):
    """(seg, table) from the annotation ``estimate_variation_in_CDS`` takes: ``gff`` what ``parse_gff_file`` or ``Annotation.from_arrays`` returns (its rows
    whose type is ``feature``, case-insensitive), or ``gbk`` what ``parse_genbank_file`` returns or its GenBankRecord (every CDS row).  ``table``: one row per
    feature in file order with start, end and strand; seg as ``segments_from_features`` of ``snp_dat.POS`` over those rows."""
    if (gbk is None) == (gff is None):
        raise ValueError("Provide either one of gbk or gff")
    if gbk is not None:
        from .gbk import GenBankRecord
        rec = gbk.get("gbk") if isinstance(gbk, dict) else gbk
        if not isinstance(rec, GenBankRecord):
            raise NotImplementedError("gbk must be what parse_genbank_file returns (or its GenBankRecord); other GenBank objects are not supported")
        if str(feature).lower() != "cds":
            raise ValueError("a GenBank record holds CDS rows only")
        rows = rec.cds
    else:
        rows = gff.gff[np.char.lower(np.asarray(gff.gff["type"]).astype(str)) == str(feature).lower()]
    table = pd.DataFrame({"start": np.asarray(rows["start"]).astype(np.int64), "end": np.asarray(rows["end"]).astype(np.int64),
                          "strand": np.asarray(rows["strand"]).astype(object)})
    return segments_from_features(snp_dat.POS, table["start"], table["end"]), table


def segments_equal(pos, g, n: int) -> np.ndarray:
    """seg (L,) int32 of ``n`` equal stretches of a genome of length ``g``: seg = min(n - 1, (pos - 1) n // g), in integers (positions are 1-based)."""
    n, g = int(n), int(g)
    if n < 1 or g < 1:
        raise ValueError("segments_equal: n and g must be positive")
    pos = np.asarray(pos, dtype=np.int64).ravel()
    return np.minimum(n - 1, (pos - 1) * n // g).astype(np.int32)


def _mirror(upper):
    """The symmetric matrix of an upper triangle (row <= column)."""
    out = np.array(upper, copy=True)
    r, c = np.triu_indices(out.shape[0], 1)
    out[c, r] = out[r, c]
    return out


@dataclass
class GeneMap:
    """n, nge, sum_lo, sum_hi int64 (S, S) and max float64 (S, S) (NaN: no pair), written where row <= column; pair uint64 (S, S) (all-ones: none) or None
    without the second walk; npairs; the segments seg (L,), the positions, thr, which, sr_dist, and the feature table when the segments came from one."""
    n: np.ndarray
    nge: np.ndarray
    sum_lo: np.ndarray
    sum_hi: np.ndarray
    max: np.ndarray
    pair: "np.ndarray | None"
    npairs: int
    seg: np.ndarray
    POS: np.ndarray
    thr: float
    which: str
    sr_dist: float
    table: "pd.DataFrame | None" = None

    @property
    def S(self) -> int:
        return int(self.n.shape[0])

    def exact_sum(self) -> np.ndarray:
        """Per cell the sum of llrint(v 2^40) as Python integers (an object array): sum_hi 2^24 + sum_lo, which int64 need not hold."""
        return self.sum_hi.astype(object) * (1 << LO_BITS) + self.sum_lo.astype(object)

    def mean(self) -> np.ndarray:
        """Per cell sum / n / 2^40, NaN where n == 0: the correctly rounded quotient of the integers.  Where |sum| < 2^53 the sum is a double already and
        the division of two doubles rounds once; elsewhere the quotient is taken in Python's integers.  Nothing passes through float before the division."""
        out = np.full(self.n.shape, np.nan)
        has = self.n > 0
        small = has & (np.abs(self.sum_hi) < (1 << (52 - LO_BITS))) & (self.sum_lo >= 0) & (self.sum_lo < (1 << 52))      # |sum_hi 2^24| < 2^52, sum_lo < 2^52
        s = (self.sum_hi[small] << LO_BITS) + self.sum_lo[small]
        out[small] = s.astype(np.float64) / self.n[small].astype(np.float64) / 2.0 ** FRAC
        for r, c in np.argwhere(has & ~small):
            num = (int(self.sum_hi[r, c]) << LO_BITS) + int(self.sum_lo[r, c])
            out[r, c] = num / (int(self.n[r, c]) << FRAC)
        return out

    def frac(self) -> np.ndarray:
        """Per cell nge / n, NaN where n == 0."""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.n > 0, self.nge.astype(np.float64) / self.n, np.nan)

    def symmetric(self, name: str) -> np.ndarray:
        """The matrix ``name`` (n, nge, sum_lo, sum_hi, max, mean, frac or exact_sum) with the upper triangle mirrored into the lower."""
        if name not in NAMES:
            raise ValueError(f"name must be one of {NAMES}, got {name!r}")
        m = getattr(self, name)
        return _mirror(m() if callable(m) else m)

    def frame(self, top=None, by: str = "nge", min_pairs: int = 1, include_diagonal: bool = False) -> pd.DataFrame:
        """One row per cell seg1 <= seg2 (seg1 < seg2 without ``include_diagonal``) of at least ``min_pairs`` (and at least one) pairs: seg1, seg2, n, nge,
        frac, mean, max, pos1, pos2 — the positions of the SNP pair behind max (the smaller SNP index first), NaN without the second walk or where it names
        none.  Ordered by ``by`` (nge, max or mean) descending, NaN last, ties by (seg1, seg2) ascending; the first ``top`` rows when given."""
        if by not in BY:
            raise ValueError(f"by must be one of {BY}, got {by!r}")
        S = self.S
        r, c = np.triu_indices(S, 0 if include_diagonal else 1)
        keep = self.n[r, c] >= max(int(min_pairs), 1)
        r, c = r[keep], c[keep]
        mean, frac = self.mean()[r, c], self.frac()[r, c]
        cols = {"nge": self.nge[r, c].astype(np.float64), "max": self.max[r, c], "mean": mean}
        key = np.where(np.isnan(cols[by]), np.inf, -cols[by])
        order = np.lexsort((c, r, key))
        if top is not None:
            order = order[:max(int(top), 0)]
        r, c = r[order], c[order]
        pos1 = pos2 = np.full(len(r), np.nan)
        if self.pair is not None:
            p = self.pair[r, c]
            ok = p != NO_PAIR
            POS = np.asarray(self.POS)
            a, b = (p >> np.uint64(32)).astype(np.int64), (p & np.uint64(0xFFFFFFFF)).astype(np.int64)
            pos1 = np.where(ok, POS[np.where(ok, a, 0)].astype(np.float64), np.nan)
            pos2 = np.where(ok, POS[np.where(ok, b, 0)].astype(np.float64), np.nan)
        return pd.DataFrame({"seg1": r.astype(np.int64), "seg2": c.astype(np.int64), "n": self.n[r, c], "nge": self.nge[r, c], "frac": frac[order], "mean": mean[order],
                             "max": self.max[r, c], "pos1": pos1, "pos2": pos2})


def gene_map(snp_dat, hdw=None, *, segments, n_segments=None, sr_dist=20000, which: str = "lr", thr=np.inf, w=None, background=None, best: bool = True,
             max_blk_sz: int = 10000, threshold: float = 0.1, quirk_mode: int = L.QUIRK_REFERENCE, engine=None, alignment_resident: bool = False, out_path=None,
             plot_path=None) -> GeneMap:
    """The segment x segment map of ``snp_dat`` under the weights ``hdw`` (computed as ``estimate_Hamming_distance_weights`` does when not given): the value of
    every SNP pair of class ``which`` (sr, lr or all, split at ``sr_dist``), block by block as ``perform_MI_computation`` visits them (``make_blocks``), folded
    on the device into the cell of the pair's two segments.  ``segments``: seg (L,) with ids in -1..n_segments-1 (-1: the SNP takes no part), or the pair
    (seg, table) of ``segments_from_annotation``; ``n_segments`` defaults to the table's rows, else to the largest id + 1.  The value is the MI, or
    MI - w[a] w[b] with ``w`` (L,); ``background`` (a ``SnpBackground``) sets w to the average product correction of class ``which`` (``apc_weights``, as
    ``apc_links`` derives it).  ``thr``: the threshold of nge.  ``best``: a second walk names the SNP pair behind every cell's maximum.  ``out_path``: the rows
    of ``GeneMap.frame(include_diagonal=True)`` as tsv, header first; ``plot_path``: ``plots.gene_map_plot``.  Nothing here changes a link table."""
    from .engine import Engine, write_table_tsv
    from .mi import make_blocks
    if which not in CLS_MASK:
        raise ValueError(f"which must be one of {WHICH}, got {which!r}")
    if snp_dat.g is None:
        raise ValueError("snp.dat$g is NULL: set the genome length first (R/BacGWES.R:338-345)")
    if w is not None and background is not None:
        raise ValueError("gene_map: give w or background, not both")
    table = None
    if isinstance(segments, tuple):
        segments, table = segments
    seg = np.ascontiguousarray(segments, dtype=np.int32).ravel()
    if len(seg) != snp_dat.nsnp:
        raise ValueError(f"gene_map: {len(seg)} segment ids for {snp_dat.nsnp} SNPs")
    if n_segments is None:
        n_segments = len(table) if table is not None else int(seg.max()) + 1
    S = int(n_segments)
    if not 1 <= S <= MAX_SEGMENTS:
        raise ValueError(f"gene_map: {S} segments, outside 1..{MAX_SEGMENTS}")
    if background is not None:
        w = apc_weights(background, which)
    if w is not None:
        w = np.ascontiguousarray(w, dtype=np.float64).ravel()
        if len(w) != snp_dat.nsnp:
            raise ValueError(f"gene_map: {len(w)} weights for {snp_dat.nsnp} SNPs")
    own = engine is None
    eng = engine or Engine(0)
    try:
        if not alignment_resident:
            eng.set_alignment(snp_dat.states)
        if hdw is None:
            hdw = eng.hamming_weights(int(snp_dat.nsnp * threshold))
        eng.set_weights(hdw)
        eng.set_snp_meta(snp_dat.r, snp_dat.uqe, snp_dat.POS, None, float(snp_dat.g))
        blocks, mask = make_blocks(snp_dat.nsnp, int(max_blk_sz)), CLS_MASK[which]
        res = eng.mi_segment_map(blocks, seg, S, float(sr_dist), mask, w, float(thr), quirk=quirk_mode)
        pair = eng.mi_segment_best(blocks, seg, S, float(sr_dist), mask, res["max"], w, quirk=quirk_mode) if best else None
        gm = GeneMap(res["n"], res["nge"], res["sum_lo"], res["sum_hi"], res["max"], pair, res["npairs"], seg, np.asarray(snp_dat.POS), float(thr), which,
                     float(sr_dist), table)
        if out_path is not None:
            fr = gm.frame(include_diagonal=True)
            with open(out_path, "w") as f:
                f.write("\t".join(fr.columns) + "\n")
            write_table_tsv(out_path, [fr[c].to_numpy() for c in fr.columns], append=True)
        if plot_path is not None:
            from .plots import gene_map_plot
            gene_map_plot(gm, plot_path, engine=eng)
    finally:
        if own:
            eng.close()
    return gm
