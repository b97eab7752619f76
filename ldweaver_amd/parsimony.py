"""Maximum parsimony on a tree, for the SNPs and the links: how often a SNP changes along the branches of a given tree — its score, its
homoplasy and consistency index — and on how many branches the two SNPs of a link change together.  Two SNPs that changed together many independent
times suggest epistasis; two that changed once, in the ancestor of a clade, are population structure.  The passes run on the device
(``Engine.tree_parsimony``, ``tree_states``, ``tree_cochanges``) over the alignment the engine holds; the tree is a ``tree.Tree`` — read from a Newick
file, or built by ``nj_tree``.  ``cochange_scan`` asks the co-change question of EVERY pair of SNPs, not of a list
(``Engine.tree_cochange_scan``, ``tree_cochange_links``)."""
from __future__ import annotations

import math

import numpy as np

GAP_MODES = {"missing": 0, "state": 1}


def _gap_mode(gaps) -> int:
    if gaps not in GAP_MODES:
        raise ValueError(f"gaps must be one of {sorted(GAP_MODES)}, got {gaps!r}")
    return GAP_MODES[gaps]


def tip_sequences(tree, seq_names) -> np.ndarray:
    """int32 [nodes]: for every tip node of ``tree`` the 0-based index of the sequence of ``seq_names`` that carries its label, -1 at the other nodes.
    Every tip label must match exactly one sequence name, other sequences are allowed (the rule of ``tree_fasta``); ValueError otherwise."""
    where = {}
    for k, s in enumerate(seq_names):
        where.setdefault(str(s), []).append(k)
    out = np.full(tree.n_nodes, -1, dtype=np.int32)
    for t, v in zip(tree.tip_label, tree.tip_node.tolist()):
        if len(where.get(str(t), ())) != 1:
            raise ValueError("Sequence names mismatch between provided tree file and fasta file")
        out[v] = where[str(t)][0]
    return out


def cochange_pvalue(branches: int, n1: int, n2: int, co: int) -> float:
    """P(X >= co) for X the overlap of two sets of ``n1`` and ``n2`` branches drawn without regard to each other among ``branches``: the upper tail of
    the hypergeometric law, in fp64 from ``math.lgamma`` terms summed smallest first.  A descriptive rank, not a test: it treats all branches alike,
    and they are not equally long — a long branch collects more changes of either SNP than a short one."""
    M, n1, n2, co = int(branches), int(n1), int(n2), int(co)
    if not (0 <= n1 <= M and 0 <= n2 <= M):
        raise ValueError(f"cochange_pvalue: {n1} and {n2} branches among {M}")
    lo, hi = max(0, n1 + n2 - M), min(n1, n2)
    if co <= lo:
        return 1.0
    if co > hi:
        return 0.0

    def lchoose(n, k):
        return math.lgamma(n + 1) - math.lgamma(k + 1) - math.lgamma(n - k + 1)

    base = lchoose(M, n2)
    terms = sorted(math.exp(lchoose(n1, x) + lchoose(M - n1, n2 - x) - base) for x in range(co, hi + 1))
    return min(1.0, math.fsum(terms))


def _engine_for(snp_dat, engine, alignment_resident, who):
    """The engine handling of ``nj_tree``: (engine, whether it is ours to close), the alignment resident on it."""
    from .engine import Engine
    if alignment_resident and engine is None:
        raise ValueError("alignment_resident=True needs the engine that holds the alignment")
    if snp_dat is None and not alignment_resident:
        raise ValueError(f"{who}: no alignment: pass snp_dat, or an engine with alignment_resident=True")
    own = engine is None
    eng = Engine(0) if own else engine
    try:
        if not alignment_resident:
            if snp_dat.states is None:
                raise ValueError("snp_dat.states is None (the alignment stayed on the device): pass its engine with alignment_resident=True")
            eng.set_alignment(snp_dat.states)
    except BaseException:
        if own:
            eng.close()
        raise
    return eng, own


def _names(snp_dat, n_seq):
    names = list(getattr(snp_dat, "seq_names", None) or [])
    return names if names else [str(k + 1) for k in range(n_seq)]


def _snp_index(snp_dat, positions, who):
    from .lr import positions_to_snp_index
    if snp_dat is None:
        raise ValueError(f"{who}: positions need snp_dat.POS")
    try:
        return positions_to_snp_index(snp_dat.POS, np.asarray(positions)).astype(np.int32)
    except ValueError:
        raise ValueError(f"{who}: a position is not a SNP position of snp_dat") from None


def snp_parsimony(tree, snp_dat=None, *, engine=None, alignment_resident=False, gaps="missing", out_path=None):
    """Per SNP of the alignment, on ``tree``: a frame of ``POS`` (``snp_dat.POS``; the 1-based SNP index without ``snp_dat``), ``score`` (the least
    number of state changes that explains the column), ``min_changes`` (distinct states at the tree's tips minus one), ``homoplasy`` (their difference)
    and ``ci`` (min_changes / score; 1.0 where the score is 0).  ``gaps``: "missing" — a tip in state N costs nothing and takes its parent's state — or
    "state": N is a fifth state.  Tips are matched to sequences by label (``tip_sequences``; sequences named 1 .. N where ``snp_dat`` has no names).
    ``engine`` / ``alignment_resident`` as for ``nj_tree``.  With ``out_path`` the frame is also written as a tab-separated file.  Needs a GPU."""
    import pandas as pd
    mode = _gap_mode(gaps)
    eng, own = _engine_for(snp_dat, engine, alignment_resident, "snp_parsimony")
    try:
        score, mn = eng.tree_parsimony(tree.parent, tip_sequences(tree, _names(snp_dat, eng.N)), mode)
    finally:
        if own:
            eng.close()
    pos = np.asarray(snp_dat.POS) if snp_dat is not None else np.arange(1, len(score) + 1, dtype=np.int32)
    df = pd.DataFrame({"POS": pos, "score": score, "min_changes": mn, "homoplasy": score - mn,
                       "ci": np.where(score == 0, 1.0, mn / np.maximum(score, 1))})
    if out_path is not None:
        df.to_csv(out_path, sep="\t", index=False)
    return df


def link_cochanges(tree, links, snp_dat=None, *, engine=None, alignment_resident=False, gaps="missing", out_path=None):
    """``links`` — a frame with ``pos1`` / ``pos2``, or the path of a top-hits file (``read_TopHits``) — with four columns appended, rows and order
    unchanged: ``changes1`` and ``changes2``, the branches of ``tree`` on which each SNP changes under the reconstruction of DESIGN.md 28,
    ``co_changes``, those on which both do, and ``co_p`` (``cochange_pvalue`` among the tree's nodes - 1 branches).  Positions map to SNPs by
    ``positions_to_snp_index``.  The other arguments as for ``snp_parsimony``.  Needs a GPU."""
    import os
    mode = _gap_mode(gaps)
    if isinstance(links, (str, bytes, os.PathLike)):
        from .output import read_TopHits
        links = read_TopHits(links)
    df = links.copy()
    a, b = _snp_index(snp_dat, df["pos1"], "link_cochanges"), _snp_index(snp_dat, df["pos2"], "link_cochanges")
    if len(df):
        eng, own = _engine_for(snp_dat, engine, alignment_resident, "link_cochanges")
        try:
            ca, cb, co = eng.tree_cochanges(tree.parent, tip_sequences(tree, _names(snp_dat, eng.N)), a, b, mode)
        finally:
            if own:
                eng.close()
    else:
        ca = cb = co = np.zeros(0, dtype=np.int32)
    seen, p = {}, []                # (many links share their three counts)
    branches = tree.n_nodes - 1
    for k in zip(ca.tolist(), cb.tolist(), co.tolist()):
        if k not in seen:
            seen[k] = cochange_pvalue(branches, *k)
        p.append(seen[k])
    df["changes1"], df["changes2"], df["co_changes"], df["co_p"] = ca, cb, co, np.asarray(p, dtype=np.float64)
    if out_path is not None:
        df.to_csv(out_path, sep="\t", index=False)
    return df


def ancestral_states(tree, positions, snp_dat=None, *, engine=None, alignment_resident=False, gaps="missing") -> np.ndarray:
    """uint8 (len(positions), nodes): the state 0..4 (A, C, G, T, N) of every node of ``tree`` for the SNP at each position, under the reconstruction
    of DESIGN.md 28.  A position listed twice gives two equal rows.  The other arguments as for ``snp_parsimony``.  Needs a GPU."""
    mode = _gap_mode(gaps)
    idx = _snp_index(snp_dat, positions, "ancestral_states")
    eng, own = _engine_for(snp_dat, engine, alignment_resident, "ancestral_states")
    try:
        return eng.tree_states(tree.parent, tip_sequences(tree, _names(snp_dat, eng.N)), idx, mode)
    finally:
        if own:
            eng.close()


# ---- the co-change scan: every pair of the SNPs that change often enough, not only the listed ones -----------------------------------------

HIST_BINS = 1024


def pick_min_co(hist, top, floor=1) -> int:
    """The smallest k in [``floor``, 1023] with sum(hist[k:]) <= ``top``, for the histogram of a co-change scan (pairs per min(co, 1023)); 1023 where even
    the open last bin holds more than ``top``: the links call sizes itself by its exact count anyway."""
    h = np.asarray(hist).astype(np.int64).ravel()
    if len(h) != HIST_BINS:
        raise ValueError(f"pick_min_co: a histogram of {len(h)} bins ({HIST_BINS} expected)")
    tail = np.cumsum(h[::-1])[::-1]                  # tail[k] = sum(hist[k:])
    for k in range(min(max(int(floor), 0), HIST_BINS - 1), HIST_BINS):
        if tail[k] <= top:
            return k
    return HIST_BINS - 1


class CochangeScan:
    """What ``cochange_scan`` returns: ``links`` (a frame of the listed pairs), ``snps`` (a frame per SNP), ``hist`` uint64 (1024,) the qualifying pairs per
    min(co, 1023), ``npairs`` the pairs looked at, ``n_qualifying`` those that passed the lift test, ``min_co`` the one the list was made with."""

    def __init__(self, links, snps, hist, npairs, n_qualifying, min_co):
        self.links, self.snps, self.hist, self.npairs, self.n_qualifying, self.min_co = links, snps, hist, int(npairs), int(n_qualifying), int(min_co)

    def __repr__(self):
        return f"CochangeScan({len(self.links)} links at co >= {self.min_co}, {self.n_qualifying} of {self.npairs} pairs qualify, {len(self.snps)} SNPs)"


def cochange_scan(tree, snp_dat=None, *, engine=None, alignment_resident=False, gaps="missing", min_changes=2, min_co=2, min_lift=0, min_len=None, top=None,
                  out_path=None):
    """Repeated co-change over EVERY pair of SNPs on ``tree``, not only the pairs a top-hits file lists.  A SNP takes part when it changes on at least
    ``min_changes`` branches (its parsimony score); a pair qualifies when its shared change branches ``co`` reach ``min_lift`` times what two independent
    branch sets of these sizes would share (co (nodes - 1) >= min_lift changes1 changes2; 0: every pair); with ``min_len`` only pairs whose circular
    distance exceeds it are looked at (needs ``snp_dat.POS`` and ``snp_dat.g``).  The qualifying pairs with co >= ``min_co`` are listed; with ``top`` the
    cut is raised by ``pick_min_co`` so that at most ``top`` are (ties in the open last bin aside).  One scan, one count, one list of exactly that size.
    Returns a ``CochangeScan``: ``links`` holds ``pos1, pos2, len`` (where positions exist; else ``snp1, snp2``, 1-based), ``changes1, changes2,
    co_changes, co_p`` (``cochange_pvalue``) and ``jaccard`` (co / (changes1 + changes2 - co)), sorted by co_p, pos1, pos2; ``snps`` holds ``POS, changes,
    best_co`` (-1: no qualifying partner), ``best_partner`` (a POS, or NA) and ``n_partners`` (the qualifying ones with co >= min_co).  ``out_path``
    writes ``links`` as a tab-separated file.  Engine handling and the tip labels as for ``snp_parsimony``.  Needs a GPU."""
    import pandas as pd
    mode = _gap_mode(gaps)
    have_pos = snp_dat is not None and getattr(snp_dat, "POS", None) is not None
    if min_len is not None and min_len >= 0 and not have_pos:
        raise ValueError("cochange_scan: min_len needs snp_dat.POS")
    mlen = -1.0 if min_len is None else float(min_len)
    eng, own = _engine_for(snp_dat, engine, alignment_resident, "cochange_scan")
    try:
        tips = tip_sequences(tree, _names(snp_dat, eng.N))
        if mlen >= 0 and not alignment_resident:             # (a resident alignment brings its meta data, or the call is refused)
            eng.set_snp_meta(snp_dat.r, snp_dat.uqe, snp_dat.POS, None, float(snp_dat.g))
        args = dict(gap_mode=mode, min_changes=int(min_changes), min_lift=int(min_lift), min_len=mlen)
        scan = eng.tree_cochange_scan(tree.parent, tips, min_co=int(min_co), **args)
        used = int(min_co) if top is None else max(int(min_co), pick_min_co(scan["hist"], int(top), floor=max(int(min_co), 0)))
        count = eng.tree_cochange_links(tree.parent, tips, min_co=used, cap=0, **args)["count"]
        got = eng.tree_cochange_links(tree.parent, tips, min_co=used, cap=count, best_in=scan["best"], **args)
    finally:
        if own:
            eng.close()
    n_snp = len(scan["changes"])
    POS = np.asarray(snp_dat.POS) if have_pos else np.arange(1, n_snp + 1, dtype=np.int32)
    a = got["a"].astype(np.int64) if count else np.zeros(0, dtype=np.int64)
    b = got["b"].astype(np.int64) if count else np.zeros(0, dtype=np.int64)
    co = got["co"].astype(np.int64) if count else np.zeros(0, dtype=np.int64)
    if used != int(min_co):         # the scan counted partners at the caller's min_co: at the raised one they are the list's own
        scan = dict(scan, nge=np.bincount(np.concatenate([a, b]), minlength=n_snp).astype(np.int64))
    c1, c2 = scan["changes"][a].astype(np.int64), scan["changes"][b].astype(np.int64)
    seen, p = {}, []                # (many links share their three counts)
    branches = tree.n_nodes - 1
    for k in zip(c1.tolist(), c2.tolist(), co.tolist()):
        if k not in seen:
            seen[k] = cochange_pvalue(branches, *k)
        p.append(seen[k])
    cols = {}
    if have_pos:
        from . import rcompat
        cols.update(pos1=POS[a], pos2=POS[b], len=rcompat.circ_len(POS[b], POS[a], float(snp_dat.g)))
    else:
        cols.update(snp1=POS[a], snp2=POS[b])
    cols.update(changes1=c1, changes2=c2, co_changes=co, co_p=np.asarray(p, dtype=np.float64), jaccard=co / np.maximum(c1 + c2 - co, 1))
    links = pd.DataFrame(cols)
    first, second = ("pos1", "pos2") if have_pos else ("snp1", "snp2")
    links = links.sort_values(["co_p", first, second], kind="stable").reset_index(drop=True)
    ps = got["partner"].astype(np.int64)
    partner = pd.array(POS[np.maximum(ps, 0)].astype(np.int64), dtype="Int64")
    partner[ps < 0] = pd.NA
    snps = pd.DataFrame({"POS": POS, "changes": scan["changes"], "best_co": scan["best"], "best_partner": partner, "n_partners": scan["nge"]})
    if out_path is not None:
        links.to_csv(out_path, sep="\t", index=False)
    return CochangeScan(links, snps, scan["hist"], scan["npairs"], scan["n_qualifying"], used)
