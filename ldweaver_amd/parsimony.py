"""Maximum parsimony on a tree, for the SNPs and the links: how often a SNP changes along the branches of a given tree — its score, its
homoplasy and consistency index — and on how many branches the two SNPs of a link change together.  Two SNPs that changed together many independent
times suggest epistasis; two that changed once, in the ancestor of a clade, are population structure.  The passes run on the device
(``Engine.tree_parsimony``, ``tree_states``, ``tree_cochanges``) over the alignment the engine holds; the tree is a ``tree.Tree`` — read from a Newick
file, or built by ``nj_tree``."""
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
