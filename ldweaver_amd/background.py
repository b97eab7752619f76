"""The MI background of every SNP (include/ldweaver_amd.h 21): per SNP and distance class the number of partners, the exact sum of their MI
in 40-bit fixed point, the largest MI and the partners above a threshold, over EVERY SNP pair of an alignment — the values the pass computes and drops —
and the average product correction of links that follows from it.  The integers are taken on the device (``Engine.mi_snp_summary``); everything in
``SnpBackground`` and ``link_apc`` is a pure host function of them.  ``apc_links`` (include/ldweaver_amd.h 22) selects links by the corrected
score over every pair instead of re-ranking a list that raw MI selected, and names every SNP's best partner by that score."""
from __future__ import annotations

import warnings
from dataclasses import dataclass

import numpy as np
import pandas as pd

from . import _lib as L

__all__ = ["snp_background", "SnpBackground", "link_apc", "apc_links", "apc_weights", "pick_threshold"]

FRAC = 40                         # fraction bits of sumq (csrc/ldw_snpsum.h SNPSUM_FRAC)
WHICH = ("sr", "lr", "all")


def exact_sum(a) -> int:
    """The sum of an int64 array as a Python integer, without int64's wrap-around: the high and the low 32 bits are summed apart (each partial sum stays
    below 2^63 for fewer than 2^31 elements)."""
    a = np.asarray(a, dtype=np.int64).ravel()
    if len(a) >= 1 << 31:
        return sum(exact_sum(a[k:k + (1 << 30)]) for k in range(0, len(a), 1 << 30))
    return (int((a >> 32).sum()) << 32) + int((a & 0xFFFFFFFF).sum())


@dataclass
class SnpBackground:
    """n, sumq, nge int64 (2, L) and max float64 (2, L) (NaN: no partner) — row 0 the short-range class (len <= sr_dist), row 1 the long-range one —,
    npairs (2,), the positions, the genome length, sr_dist and the two thresholds of nge."""
    n: np.ndarray
    sumq: np.ndarray
    max: np.ndarray
    nge: np.ndarray
    npairs: np.ndarray
    POS: np.ndarray
    g: float
    sr_dist: float
    thr: tuple

    def _sums(self, which):
        if which not in WHICH:
            raise ValueError(f"which must be one of {WHICH}, got {which!r}")
        if which == "all":
            return self.sumq.sum(axis=0), self.n.sum(axis=0)
        c = WHICH.index(which)
        return self.sumq[c], self.n[c]

    def mean(self, which: str = "lr") -> np.ndarray:
        """Per SNP the mean MI with its partners of the class: sumq / n / 2^40, NaN where n == 0.  "all" adds the two classes first."""
        s, n = self._sums(which)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n > 0, s.astype(np.float64) / n / 2.0 ** FRAC, np.nan)

    def overall_mean(self, which: str = "lr") -> float:
        """The mean MI over the pairs of the class: sum of sumq / sum of n (every pair counts once at each of its SNPs); NaN without a pair.  The sum over
        the SNPs is taken in Python's integers (``exact_sum``): a SNP's sumq stays below 2^62, their sum over an alignment does not stay below 2^63."""
        if which not in WHICH:
            raise ValueError(f"which must be one of {WHICH}, got {which!r}")
        cls = (0, 1) if which == "all" else (WHICH.index(which),)
        tot = sum(exact_sum(self.n[c]) for c in cls)
        return float(sum(exact_sum(self.sumq[c]) for c in cls) / tot / 2.0 ** FRAC) if tot else float("nan")

    def hubs(self, which: str = "lr", top: int = 20) -> pd.DataFrame:
        """The ``top`` SNPs of the largest mean MI with their partners of the class, largest first (ties by position order): snp, pos, n, mean."""
        s, n = self._sums(which)
        m = self.mean(which)
        order = np.argsort(-np.where(np.isnan(m), -np.inf, m), kind="stable")[:max(int(top), 0)]
        order = order[~np.isnan(m[order])]
        return pd.DataFrame({"snp": order.astype(np.int64), "pos": np.asarray(self.POS)[order], "n": n[order], "mean": m[order]})

    def frame(self) -> pd.DataFrame:
        return pd.DataFrame({"pos": np.asarray(self.POS), "n_sr": self.n[0], "mean_sr": self.mean("sr"), "max_sr": self.max[0], "nge_sr": self.nge[0],
                             "n_lr": self.n[1], "mean_lr": self.mean("lr"), "max_lr": self.max[1], "nge_lr": self.nge[1]})


def snp_background(snp_dat, hdw=None, *, sr_dist=20000, thr=(np.inf, np.inf), max_blk_sz: int = 10000, threshold: float = 0.1,
                   quirk_mode: int = L.QUIRK_REFERENCE, engine=None, alignment_resident: bool = False, out_path=None, plot_path=None) -> SnpBackground:
    """The MI background of ``snp_dat`` under the weights ``hdw`` (computed as ``estimate_Hamming_distance_weights`` does when not given): the MI of every
    SNP pair, block by block as ``perform_MI_computation`` visits them (``make_blocks``), summed on the device per SNP and distance class.  ``thr``: the
    two thresholds (short range, long range) of the ``nge`` counts.  ``out_path``: the rows of ``SnpBackground.frame()`` as tsv, header first;
    ``plot_path``: ``plots.snp_background_plot``.  Nothing here changes a link table."""
    from .engine import Engine, write_table_tsv
    from .mi import make_blocks
    if snp_dat.g is None:
        raise ValueError("snp.dat$g is NULL: set the genome length first (R/BacGWES.R:338-345)")
    g = float(snp_dat.g)
    th = tuple(float(t) for t in np.asarray(thr, dtype=np.float64).reshape(2))
    own = engine is None
    eng = engine or Engine(0)
    try:
        if not alignment_resident:
            eng.set_alignment(snp_dat.states)
        if hdw is None:
            hdw = eng.hamming_weights(int(snp_dat.nsnp * threshold))
        eng.set_weights(hdw)
        eng.set_snp_meta(snp_dat.r, snp_dat.uqe, snp_dat.POS, None, g)
        res = eng.mi_snp_summary(make_blocks(snp_dat.nsnp, int(max_blk_sz)), float(sr_dist), th, quirk=quirk_mode)
        bg = SnpBackground(res["n"], res["sumq"], res["max"], res["nge"], res["npairs"], np.asarray(snp_dat.POS), g, float(sr_dist), th)
        if out_path is not None:
            fr = bg.frame()
            with open(out_path, "w") as f:
                f.write("\t".join(fr.columns) + "\n")
            write_table_tsv(out_path, [fr[c].to_numpy() for c in fr.columns], append=True)
        if plot_path is not None:
            from .plots import snp_background_plot
            snp_background_plot(bg, plot_path, engine=eng)
    finally:
        if own:
            eng.close()
    return bg


CLS_MASK = {"sr": 1, "lr": 2, "all": 3}     # ldw_mi_score_scan's class mask of ``which``
NBINS = 4096
BUCKET_OFF = (1023 - 20) << 7              # csrc/ldw_epi.h: bucket B >= 1 starts at the double with bits (B + BUCKET_OFF) << 45
CAP_LIMIT = 1 << 26


def pick_threshold(hist, top: int):
    """The threshold of ``apc_links`` from the scan's histogram, a pure function: with cum(B) the pairs in the buckets >= B, B* is the largest B >= 1 with
    cum(B) >= top, else 1.  Returns (thr, cap): thr the lower edge of bucket B*, the double with bits (B* + ((1023 - 20) << 7)) << 45, and cap = cum(B*).
    Bucket edges are monotone in the value, so exactly cap pairs have a score >= thr.  Bucket 0 is never taken: scores below 2^-20 are never listed."""
    h = np.asarray(hist).astype(np.uint64).astype(object)                      # Python integers: no wrap-around
    if h.shape != (NBINS,):
        raise ValueError(f"pick_threshold: the histogram has shape {h.shape}, not ({NBINS},)")
    cum = np.cumsum(h[::-1])[::-1]
    reach = [B for B in range(1, NBINS) if cum[B] >= top]
    B = max(reach) if reach else 1
    thr = float(np.array([(B + BUCKET_OFF) << 45], dtype=np.int64).view(np.float64)[0])
    return thr, int(cum[B])


def apc_weights(background: "SnpBackground", which: str = "lr") -> np.ndarray:
    """The per-SNP vector of the average product correction: w = mean(which) / sqrt(overall_mean(which)), so that w[a] w[b] = mean(a) mean(b) / overall.
    0 where the mean is NaN (such a SNP has no pair in the class).  ValueError when the overall mean is not positive."""
    overall = background.overall_mean(which)
    if not overall > 0:
        raise ValueError(f"apc_weights: the overall mean MI of class {which!r} is {overall}: the correction needs a positive one")
    m = background.mean(which)
    return np.where(np.isnan(m), 0.0, m / np.sqrt(overall))


def apc_links(snp_dat, hdw=None, *, background: "SnpBackground | None" = None, top: int = 1000, which: str = "lr", sr_dist=20000, max_blk_sz: int = 10000,
              threshold: float = 0.1, quirk_mode: int = L.QUIRK_REFERENCE, engine=None, alignment_resident: bool = False, out_path=None):
    """The ``top`` links of class ``which`` by the APC-corrected score mi_apc = MI - w[a] w[b], selected over EVERY SNP pair — not re-ranked from a list
    selected by raw MI, as ``link_apc`` does — and every SNP's best partner by that score.  ``background=None`` runs ``snp_background`` first, on the same
    engine.  The flow: ``Engine.mi_score_scan`` (histogram of the score, best score per SNP), ``pick_threshold``, ``Engine.mi_score_links`` with that
    threshold, capacity and the scan's best scores; the host sorts by score descending, ties by (a, b) ascending, and trims to ``top``.  Scores below 2^-20
    are never listed (bucket 0 of the histogram holds them together with the negatives), so fewer than ``top`` rows may come back; a threshold bucket that
    holds more than 2^26 pairs raises ValueError: ask for a smaller ``top``.
    Returns (links, partners): ``links`` with pos1 (the to-SNP), pos2 (the from-SNP), len, MI, bg1, bg2 (the background means of the two), apc = w w and
    mi_apc, the device's score; ``partners`` one row per SNP: pos, best (its largest score, NaN without a partner in the class), partner_pos (NaN where
    none), partner_snp (-1 where none).  ``out_path``: ``links`` as tsv, header first.  Nothing here changes a link table."""
    from . import rcompat
    from .engine import Engine, write_table_tsv
    from .mi import make_blocks
    if which not in CLS_MASK:
        raise ValueError(f"which must be one of {WHICH}, got {which!r}")
    own = engine is None
    eng = engine or Engine(0)
    try:
        if background is None:
            background = snp_background(snp_dat, hdw, sr_dist=sr_dist, max_blk_sz=max_blk_sz, threshold=threshold, quirk_mode=quirk_mode, engine=eng,
                                        alignment_resident=alignment_resident)
        else:
            if snp_dat.g is None:
                raise ValueError("snp.dat$g is NULL: set the genome length first (R/BacGWES.R:338-345)")
            if not alignment_resident:
                eng.set_alignment(snp_dat.states)
            if hdw is None:
                hdw = eng.hamming_weights(int(snp_dat.nsnp * threshold))
            eng.set_weights(hdw)
            eng.set_snp_meta(snp_dat.r, snp_dat.uqe, snp_dat.POS, None, float(snp_dat.g))
        w = apc_weights(background, which)
        if len(w) != snp_dat.nsnp:
            raise ValueError(f"apc_links: the background has {len(w)} SNPs, snp_dat {snp_dat.nsnp}")
        blocks, mask = make_blocks(snp_dat.nsnp, int(max_blk_sz)), CLS_MASK[which]
        scan = eng.mi_score_scan(blocks, float(sr_dist), mask, w, quirk=quirk_mode)
        thr, cap = pick_threshold(scan["hist"], int(top))
        if cap > CAP_LIMIT:
            raise ValueError(f"apc_links: {cap} pairs share the threshold bucket of top = {top} (more than 2^26): ask for a smaller top")
        got = eng.mi_score_links(blocks, float(sr_dist), mask, w, thr, cap, best_in=scan["best"], quirk=quirk_mode)
        assert got["count"] == cap, (got["count"], cap)                       # bucket edges are monotone in the value
    finally:
        if own:
            eng.close()
    POS = np.asarray(snp_dat.POS)
    if cap:
        a, b, mi, sc = (got[k] for k in ("a", "b", "mi", "score"))
        order = np.lexsort((b, a, -sc))[:max(int(top), 0)]
        a, b, mi, sc = a[order], b[order], mi[order], sc[order]
    else:
        a = b = np.zeros(0, dtype=np.int32)
        mi = sc = np.zeros(0)
    m = background.mean(which)
    pos1, pos2 = POS[b].astype(np.float64), POS[a].astype(np.float64)
    links = pd.DataFrame({"pos1": pos1, "pos2": pos2, "len": rcompat.circ_len(pos1, pos2, float(snp_dat.g)), "MI": mi, "bg1": m[b], "bg2": m[a],
                          "apc": w[a] * w[b], "mi_apc": sc})
    ps = got["partner"].astype(np.int64)
    partners = pd.DataFrame({"pos": POS, "best": scan["best"], "partner_pos": np.where(ps >= 0, POS[np.maximum(ps, 0)].astype(np.float64), np.nan),
                             "partner_snp": ps})
    partners.attrs["cap"], partners.attrs["thr"] = cap, thr
    if out_path is not None:
        with open(out_path, "w") as f:
            f.write("\t".join(links.columns) + "\n")
        write_table_tsv(out_path, [links[c].to_numpy() for c in links.columns], append=True)
    return links, partners


def _mi_column(df):
    for name in ("MI", "mi", "mi_all"):
        if name in df.columns:
            return name
    raise ValueError("link_apc: the links have no MI column (MI, mi or mi_all)")


def link_apc(links, background: SnpBackground, snp_dat=None, *, which: str = "lr") -> pd.DataFrame:
    """``links`` — a frame with ``pos1`` / ``pos2`` and an MI column, or the path of a top-hits file (``read_TopHits``), as ``link_lineage_mi`` takes them —
    with four columns appended, rows and order unchanged: ``bg1`` / ``bg2`` the background means (``background.mean(which)``) of the two SNPs, ``apc`` =
    bg1 bg2 / ``background.overall_mean(which)`` and ``mi_apc`` = MI - apc, the average product correction.  Positions map to SNPs by
    ``positions_to_snp_index`` on ``snp_dat.POS`` (the background's own positions without ``snp_dat``); an unknown position raises.  ``apc`` is NaN, with
    one warning, when the overall mean is 0."""
    import os
    from types import SimpleNamespace
    from .parsimony import _snp_index
    if isinstance(links, (str, bytes, os.PathLike)):
        from .output import read_TopHits
        links = read_TopHits(links)
    df = links.copy()
    mi = df[_mi_column(df)].to_numpy(dtype=np.float64)
    src = snp_dat if snp_dat is not None else SimpleNamespace(POS=np.asarray(background.POS))
    a, b = _snp_index(src, df["pos1"], "link_apc"), _snp_index(src, df["pos2"], "link_apc")
    m = background.mean(which)
    if len(m) != len(np.asarray(src.POS)):
        raise ValueError(f"link_apc: the background has {len(m)} SNPs, snp_dat {len(np.asarray(src.POS))}")
    overall = background.overall_mean(which)
    bg1, bg2 = m[a], m[b]
    if overall == 0:
        warnings.warn("link_apc: the overall mean MI is 0: apc is NaN", RuntimeWarning, stacklevel=2)
        apc = np.full(len(df), np.nan)
    else:
        apc = bg1 * bg2 / overall
    df["bg1"], df["bg2"], df["apc"], df["mi_apc"] = bg1, bg2, apc, mi - apc
    return df
