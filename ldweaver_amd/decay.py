"""LD decay (include/ldweaver_amd.h 20): the histogram, circular distance bin x MI bucket, of EVERY SNP pair of an alignment —
the values the pass computes and drops — and what follows from it on the host: quantile curves per distance, the MI background at long range
and a suggestion for ``sr_dist``.  The histogram is taken on the device (``Engine.mi_profile``); everything in ``LDDecay`` is a pure host
function of its integers."""
from __future__ import annotations

import math
import warnings
from dataclasses import dataclass

import numpy as np
import pandas as pd

from . import _lib as L

__all__ = ["ld_decay", "LDDecay", "default_cuts", "bucket_lo"]

NBINS = 4096                      # the engine's MI buckets (csrc/ldw_internal.h NBINS)
BUCKET_OFF = (1023 - 20) << 7     # csrc/ldw_epi.h


def bucket_lo(B):
    """Lower edge of the engine's MI bucket(s) B >= 1 (csrc/ldw_epi.h bucket_lo): the double with the bits (B + BUCKET_OFF) << 45.  B = 4096 gives the
    edge past the last bucket."""
    return ((np.asarray(B, dtype=np.int64) + BUCKET_OFF) << 45).view(np.float64)


def bin_edges(mi_shift: int):
    """(lo, hi) of the NB = 4096 >> mi_shift MI bins: bin j holds the engine buckets j << mi_shift .. ((j + 1) << mi_shift) - 1; lo of bin 0 is 0.0 (it also
    holds the negatives) and hi of the last bin is +inf (it also holds everything past the top)."""
    nb = NBINS >> mi_shift
    e = bucket_lo(np.arange(nb + 1, dtype=np.int64) << mi_shift)
    lo, hi = e[:-1].copy(), e[1:].copy()
    lo[0], hi[-1] = 0.0, np.inf
    return lo, hi


def default_cuts(g, n_bins: int = 48) -> np.ndarray:
    """Cuts for ``n_bins`` distance bins on a genome of length g: n_bins - 1 integers geometrically spaced from 100 up to, but not including, g / 2, with
    duplicates removed (so a short genome gets fewer bins; none at all when g / 2 <= 100)."""
    half = float(g) / 2
    if n_bins < 2 or not half > 100:
        return np.zeros(0)
    c = np.unique(np.rint(np.geomspace(100.0, half, int(n_bins) - 1, endpoint=False)))
    return c[c < half]


def _rank_bin(counts: np.ndarray, q: float) -> int:
    """The bin that holds rank ceil(q n) (1-based, at least 1) of the n values counted in ``counts``; -1 when n = 0."""
    n = int(counts.sum())
    if n == 0:
        return -1
    rank = min(max(int(math.ceil(q * n)), 1), n)
    return int(np.searchsorted(np.cumsum(counts.astype(np.int64)), rank, side="left"))


@dataclass
class LDDecay:
    """hist (n_cut + 1, NB) uint64, max (n_cut + 1,) (NaN: empty bin), cuts (n_cut,), the genome length, mi_shift, the number of pairs.  Distance bin k holds
    the pairs with cuts[k - 1] < len <= cuts[k]."""
    hist: np.ndarray
    max: np.ndarray
    cuts: np.ndarray
    g: float
    mi_shift: int
    n_pairs: int

    @property
    def len_lo(self):
        return np.concatenate([[0.0], np.asarray(self.cuts, dtype=np.float64)])

    @property
    def len_hi(self):
        return np.concatenate([np.asarray(self.cuts, dtype=np.float64), [float(self.g) / 2]])

    @property
    def bin_pairs(self):
        return self.hist.astype(np.int64).sum(axis=1)

    def _quantile_of(self, counts, q):
        lo, hi = bin_edges(self.mi_shift)
        j = _rank_bin(counts, q)
        return (np.nan, np.nan) if j < 0 else (float(lo[j]), float(hi[j]))

    def quantile(self, q: float):
        """(lo, hi) per distance bin: the edges of the MI bin that holds rank ceil(q n) of the bin's n pairs, so that order statistic lies in [lo, hi).
        NaN for an empty bin."""
        out = np.array([self._quantile_of(row, q) for row in self.hist], dtype=np.float64).reshape(-1, 2)
        return out[:, 0], out[:, 1]

    def mean_estimate(self):
        """Per distance bin the mean of the MI bins' midpoints (the last bin: its lower edge) weighted by their counts.  An ESTIMATE: it is within the width of
        an MI bin (a factor 2^(2^mi_shift / 128) from edge to edge) of the true mean of the non-negative values, and counts every negative value as the
        midpoint of bin 0; it is never a sum taken on the device.  NaN for an empty bin."""
        lo, hi = bin_edges(self.mi_shift)
        mid = np.where(np.isfinite(hi), 0.5 * (lo + np.where(np.isfinite(hi), hi, 0.0)), lo)
        n = self.bin_pairs
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(n > 0, (self.hist.astype(np.float64) * mid[None, :]).sum(axis=1) / n, np.nan)

    def _background_bins(self, from_len):
        from_len = float(self.g) / 4 if from_len is None else float(from_len)
        return self.len_lo >= from_len

    def background(self, q: float = 0.95, from_len=None):
        """(lo, hi) of the same quantile over the pairs of all distance bins whose lower cut is >= from_len (default g / 4): the MI level of unlinked
        pairs.  ValueError when no such bin holds a pair."""
        pooled = self.hist[self._background_bins(from_len)].astype(np.int64).sum(axis=0)
        if pooled.sum() == 0:
            raise ValueError("no pair lies in a distance bin at or beyond from_len: add cuts there")
        return self._quantile_of(pooled, q)

    def suggest_sr_dist(self, q: float = 0.95, factor: float = 2.0, from_len=None, min_pairs: int = 100):
        """The upper cut of the LAST distance bin with at least ``min_pairs`` pairs whose q-quantile (its lo) exceeds ``factor`` x the background's lo: where
        the MI of pairs at that distance stops standing out of the background.  0.0 when no bin does; None, with a warning, when that bin is the last one
        (LD reaches past every cut)."""
        bg = self.background(q, from_len)[0]
        qlo, _ = self.quantile(q)
        with np.errstate(invalid="ignore"):
            above = (self.bin_pairs >= int(min_pairs)) & (qlo > factor * bg)
        if not above.any():
            return 0.0
        k = int(np.flatnonzero(above)[-1])
        if k == len(self.hist) - 1:
            warnings.warn("the last distance bin still stands out of the background: no cut bounds the reach of LD", RuntimeWarning, stacklevel=2)
            return None
        return float(self.cuts[k])

    def frame(self, quantiles=(0.5, 0.95, 0.99)) -> pd.DataFrame:
        cols = {"len_lo": self.len_lo, "len_hi": self.len_hi, "n_pairs": self.bin_pairs}
        for q in quantiles:
            cols[f"q{100 * q:g}"] = self.quantile(q)[0]
        cols["max"] = np.asarray(self.max, dtype=np.float64)
        cols["mean_est"] = self.mean_estimate()
        return pd.DataFrame(cols)


def ld_decay(snp_dat, hdw=None, *, cuts=None, n_bins: int = 48, mi_shift: int = 3, max_blk_sz: int = 10000, threshold: float = 0.1,
             quirk_mode: int = L.QUIRK_REFERENCE, engine=None, alignment_resident: bool = False, out_path=None, plot_path=None) -> LDDecay:
    """The LD-decay profile of ``snp_dat`` under the weights ``hdw`` (computed as ``estimate_Hamming_distance_weights`` does when not given): the MI of
    every SNP pair, block by block as ``perform_MI_computation`` visits them (``make_blocks``), binned on the device by circular distance (``cuts``,
    default ``default_cuts(g, n_bins)``) and MI bucket.  ``out_path``: the rows of ``LDDecay.frame()`` as tsv, header first; ``plot_path``:
    ``plots.ld_decay_plot``.  Nothing here changes a link table."""
    from .engine import Engine, write_table_tsv
    from .mi import make_blocks
    if snp_dat.g is None:
        raise ValueError("snp.dat$g is NULL: set the genome length first (R/BacGWES.R:338-345)")
    g = float(snp_dat.g)
    cu = default_cuts(g, n_bins) if cuts is None else np.asarray(cuts, dtype=np.float64).ravel()
    own = engine is None
    eng = engine or Engine(0)
    try:
        if not alignment_resident:
            eng.set_alignment(snp_dat.states)
        if hdw is None:
            hdw = eng.hamming_weights(int(snp_dat.nsnp * threshold))
        eng.set_weights(hdw)
        eng.set_snp_meta(snp_dat.r, snp_dat.uqe, snp_dat.POS, None, g)
        res = eng.mi_profile(make_blocks(snp_dat.nsnp, int(max_blk_sz)), cu, mi_shift=mi_shift, quirk=quirk_mode)
        dec = LDDecay(res["hist"], res["max"], cu, g, int(mi_shift), res["n_pairs"])
        if out_path is not None:
            fr = dec.frame()
            with open(out_path, "w") as f:
                f.write("\t".join(fr.columns) + "\n")
            write_table_tsv(out_path, [fr[c].to_numpy() for c in fr.columns], append=True)
        if plot_path is not None:
            from .plots import ld_decay_plot
            ld_decay_plot(dec, plot_path, engine=eng)
    finally:
        if own:
            eng.close()
    return dec
