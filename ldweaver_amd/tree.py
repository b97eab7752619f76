"""The tree view of the reference (R/preptrees.R): ``view_tree`` draws the alleles of the chosen link SNPs, column by column, and the metadata under
the tree of the isolates.  DESIGN.md 23.

The selection of links, SNP columns, FASTA rows and metadata rows is the reference's (:67-179), restated step by step.  The tree handling is ours and
needs neither ape nor phytools: ``read_newick`` parses iteratively, ``midpoint_root`` finds the root by two sweeps in O(tips) where
``phytools::midpoint.root`` builds the matrix of all tip-to-tip distances, ``ladderize`` orders the children.  The picture is ours too: the tree as
bars in 1/16 pixel and the bands as area-weighted means of their tips' colours, rendered on the device (``Engine.plot_tree``, include/ldweaver_amd.h
15); the host draws the band labels, the title and the two legends.

Without a tree file the tree is built here: ``nj_tree`` joins neighbours on the device (``Engine.nj_tree``) over the Hamming distances of
the alignment the engine holds, or over a distance matrix; ``write_newick`` writes any ``Tree`` so that ``read_newick`` returns it bit for bit."""
from __future__ import annotations

import math
import os
import re
import warnings
from dataclasses import dataclass

import numpy as np

from .network import hue_palette

MISSING_LEVEL = 255
MISSING_RGB = 0xD3D3D3
TREE_RGB = 0x000000
MAX_CANVAS = 8192


@dataclass
class Tree:
    """A rooted tree.  Nodes are numbered in depth-first order, a parent before its children and the children of a node in their order (file order
    after ``read_newick``), so ``parent[v] < v`` and the tips ascend by node in the order of the figure.  Tips keep their index of the file."""
    parent: np.ndarray      # int32 [nodes]; -1 at the root (node 0)
    length: np.ndarray      # float64 [nodes]: the branch to the parent; 0 at the root
    tip_label: list         # [tips] str, in file order
    tip_node: np.ndarray    # int32 [tips]: the node of every tip
    child_ptr: np.ndarray   # int32 [nodes + 1]: the children of v are child_idx[child_ptr[v] : child_ptr[v + 1]], in order
    child_idx: np.ndarray   # int32 [nodes - 1]
    support: np.ndarray = None   # int32 [nodes], or None: how many bootstrap replicates have the branch to the parent; -1 where there is no count
    n_replicates: int = None     # the replicates ``support`` counts, where the tree knows (a Newick file does not say)

    @property
    def n_nodes(self) -> int:
        return len(self.parent)

    @property
    def n_tips(self) -> int:
        return len(self.tip_label)

    def children(self, v: int) -> np.ndarray:
        return self.child_idx[self.child_ptr[v]:self.child_ptr[v + 1]]

    def tip_order(self) -> np.ndarray:
        """The tips (file indices) in depth-first order: the order of the figure, left to right."""
        return np.argsort(self.tip_node, kind="stable").astype(np.int32)

    def depths(self) -> np.ndarray:
        d = np.zeros(self.n_nodes, dtype=np.float64)
        par, ln = self.parent.tolist(), self.length.tolist()
        out = [0.0] * self.n_nodes
        for v in range(1, self.n_nodes):
            out[v] = out[par[v]] + ln[v]
        d[:] = out
        return d


def _build(root, kids, elen, tip_of, tip_label, esup=None, n_replicates=None) -> Tree:
    """The Tree of the rooted structure ``kids`` (node -> its children in order; any hashable ids), ``elen(child)`` the length of the branch above a
    child, ``tip_of`` node -> tip index (absent or -1: internal): renumbered depth-first without recursion.  ``esup(child)``, where given: the support
    of that branch (-1: none)."""
    order, parent = [], []
    stack = [(root, -1)]
    while stack:
        v, p = stack.pop()
        me = len(order)
        order.append(v)
        parent.append(p)
        for u in reversed(kids(v)):
            stack.append((u, me))
    n = len(order)
    length = np.zeros(n, dtype=np.float64)
    support = None if esup is None else np.full(n, -1, dtype=np.int32)
    tip_node = np.full(len(tip_label), -1, dtype=np.int32)
    for me, v in enumerate(order):
        if me:
            length[me] = elen(v)
            if esup is not None:
                support[me] = esup(v)
        t = tip_of(v)
        if t >= 0:
            tip_node[t] = me
    par = np.asarray(parent, dtype=np.int32)
    cnt = np.bincount(par[1:], minlength=n) if n > 1 else np.zeros(n, dtype=np.int64)
    ptr = np.zeros(n + 1, dtype=np.int32)
    ptr[1:] = np.cumsum(cnt)
    idx = (np.argsort(par[1:], kind="stable") + 1).astype(np.int32) if n > 1 else np.zeros(0, dtype=np.int32)   # ascending node = the order given
    return Tree(par, length, list(tip_label), tip_node, ptr, idx, support, n_replicates if support is not None else None)


# ---- Newick ---------------------------------------------------------------------------------------------------------------------------------------

_WS = re.compile(rb"[ \t\r\n]*")
_PLAIN = re.compile(rb"[^()\[\],:;' \t\r\n]*")
_NUM = re.compile(rb"[-+]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][-+]?[0-9]+)?")


def parse_newick(data: bytes) -> Tree:
    """``read_newick`` on the bytes of a file."""
    n = len(data)

    def skip(i):
        while True:
            i = _WS.match(data, i).end()
            if i < n and data[i] == 0x5B:       # [comment]
                j = data.find(b"]", i + 1)
                if j < 0:
                    raise ValueError(f"Newick: the comment opened at byte {i} is not closed")
                i = j + 1
            else:
                return i

    def label(i):
        i = skip(i)
        if i < n and data[i] == 0x27:           # 'quoted', '' is a quote
            start, j, parts = i, i + 1, []
            while True:
                k = data.find(b"'", j)
                if k < 0:
                    raise ValueError(f"Newick: the quoted label opened at byte {start} is not closed")
                parts.append(data[j:k])
                if k + 1 < n and data[k + 1] == 0x27:
                    parts.append(b"'")
                    j = k + 2
                else:
                    return b"".join(parts), k + 1
        m = _PLAIN.match(data, i)
        return m.group(0), m.end()

    def branch(i):
        i = skip(i)
        if i < n and data[i] == 0x3A:           # :length
            j = skip(i + 1)
            m = _NUM.match(data, j)
            if not m:
                raise ValueError(f"Newick: no branch length at byte {j}")
            return float(m.group(0)), m.end()
        return 0.0, i

    parent, length, labels, is_tip = [], [], [], []
    support = {}                                # internal node -> the plain non-negative integer it is labelled with
    stack, expect, i = [], True, 0
    while True:
        i = skip(i)
        if i >= n:
            raise ValueError(f"Newick: the text ends at byte {i} before the closing ';'")
        c = data[i]
        if expect:
            node = len(parent)
            parent.append(stack[-1] if stack else -1)
            length.append(0.0)
            labels.append(None)
            if c == 0x28:                       # (
                is_tip.append(False)
                stack.append(node)
                i += 1
                continue
            is_tip.append(True)
            lab, j = label(i)
            if not lab:
                raise ValueError(f"Newick: a tip without a label at byte {i}")
            labels[node] = lab
            length[node], i = branch(j)
            expect = False
        elif c == 0x2C:                         # ,
            if not stack:
                raise ValueError(f"Newick: ',' outside parentheses at byte {i}")
            expect = True
            i += 1
        elif c == 0x29:                         # )
            if not stack:
                raise ValueError(f"Newick: ')' without '(' at byte {i}")
            node = stack.pop()
            k = skip(i + 1)
            lab, j = label(k)                   # an internal label is a support count where it is a plain integer, else read and ignored
            if node and lab.isdigit() and data[k] != 0x27 and int(lab) < 2 ** 31:
                support[node] = int(lab)
            length[node], i = branch(j)
        elif c == 0x3B:                         # ;
            if stack:
                raise ValueError(f"Newick: ';' at byte {i} with {len(stack)} open '('")
            break
        else:
            raise ValueError(f"Newick: unexpected character {chr(c)!r} at byte {i}")
    tips = [v for v in range(len(parent)) if is_tip[v]]
    tip_label = [labels[v].decode("utf-8", "surrogateescape") for v in tips]
    if len(tips) < 2:
        raise ValueError(f"Newick: a tree of {len(tips)} tips (at least two are needed)")
    if len(set(tip_label)) != len(tip_label):
        seen = set()
        dup = next(s for s in tip_label if s in seen or seen.add(s))
        raise ValueError(f"Newick: the tip label {dup!r} occurs more than once")
    n_nodes = len(parent)
    par = np.asarray(parent, dtype=np.int32)     # creation order is depth-first order already
    ln = np.asarray(length, dtype=np.float64)
    ln[0] = 0.0                                  # (a length after the outermost parenthesis has no branch to sit on)
    cnt = np.bincount(par[1:], minlength=n_nodes)
    ptr = np.zeros(n_nodes + 1, dtype=np.int32)
    ptr[1:] = np.cumsum(cnt)
    idx = (np.argsort(par[1:], kind="stable") + 1).astype(np.int32)
    sup = None
    if support:
        sup = np.full(n_nodes, -1, dtype=np.int32)
        sup[list(support)] = list(support.values())
    return Tree(par, ln, tip_label, np.asarray(tips, dtype=np.int32), ptr, idx, sup)


def read_newick(path) -> Tree:
    """The first tree of a Newick file: nested parentheses, multifurcations, unquoted labels, 'quoted labels' with '' for a quote, ``:length`` in
    decimal or exponent form (missing: 0.0), ``[comments]`` skipped, a closing ``;``.  An internal label that is a plain non-negative integer (unquoted,
    below 2^31, not at the root) is the support of the branch above its node and goes into ``support`` (-1 elsewhere; None when the file has no such
    label); any other internal label is read and ignored.  Iterative: a caterpillar of any depth parses.  Malformed text raises ValueError naming the
    byte offset; so do fewer than two tips and a repeated tip label."""
    with open(path, "rb") as fh:
        return parse_newick(fh.read())


_NEEDS_QUOTES = re.compile(r"[()\[\],:;' \t\r\n]")


def _newick_label(s: str) -> str:
    """A label as ``parse_newick`` reads it back: plain when it holds none of ``()[],:;'`` and no white space, else 'quoted' with '' for a quote."""
    if not s:
        raise ValueError("write_newick: an empty tip label cannot be read back")
    return "'" + s.replace("'", "''") + "'" if _NEEDS_QUOTES.search(s) else s


def write_newick(tree: Tree, path=None) -> str:
    """The tree as one line of Newick text, returned and, with ``path``, written there: children in their order, every branch length as
    ``repr(float)`` (the shortest text that reads back as the same double), tip labels quoted where they need it, no length at the root.  Internal
    nodes are labelled with their support where the tree has one that is >= 0, as in ``)87:0.25``, and not otherwise.  ``read_newick`` of the result has
    the same parent array, labels, lengths and support (a support array without a single count reads back as None)."""
    ptr, idx, ln = tree.child_ptr.tolist(), tree.child_idx.tolist(), tree.length.tolist()
    sup = None if tree.support is None else tree.support.tolist()
    lab = {int(v): _newick_label(str(tree.tip_label[t])) for t, v in enumerate(tree.tip_node.tolist())}
    parts, stack = [], [(0, 0)]
    while stack:
        v, k = stack.pop()
        nk = ptr[v + 1] - ptr[v]
        if k < nk:                              # open the node or go on to its next child
            parts.append("(" if k == 0 else ",")
            stack.append((v, k + 1))
            stack.append((idx[ptr[v] + k], 0))
            continue
        parts.append(")" if nk else lab[v])
        if v:
            if nk and sup is not None and sup[v] >= 0:
                parts.append(str(sup[v]))
            parts.append(":" + repr(float(ln[v])))
    text = "".join(parts) + ";\n"
    if path is not None:
        with open(path, "wb") as fh:
            fh.write(text.encode("utf-8", "surrogateescape"))
    return text


# ---- neighbour joining ------------------------------------------------------------------------------------------------------------------

def nj_clamp(parent: np.ndarray, length: np.ndarray) -> np.ndarray:
    """The lengths of ``Engine.nj_tree`` without negative branches: where one branch of a join is negative it becomes 0 and its sibling gets the sum
    of the two, which is d_ab (la + lb: to the last bit where the lengths are dyadic, else within one rounding); a negative branch at the root
    becomes 0.  Returns a copy."""
    out = np.array(length, dtype=np.float64)
    n = (len(parent) + 2) // 2
    kids = {}
    for v in range(2 * n - 3):
        kids.setdefault(int(parent[v]), []).append(v)
    for u in range(n, 2 * n - 3):
        a, b = kids[u]
        la, lb = float(out[a]), float(out[b])
        if la < 0:
            out[a], out[b] = 0.0, la + lb
        elif lb < 0:
            out[a], out[b] = la + lb, 0.0
    for v in kids[2 * n - 3]:
        if out[v] < 0:
            out[v] = 0.0
    return out


def bootstrap_multiplicities(L: int, B: int, seed: int = 0) -> np.ndarray:
    """The column multiplicities of B Felsenstein bootstrap replicates of an alignment of L SNP columns, int32 (B, L), every row adding up to L:
    ``rng = np.random.default_rng(seed)`` and then, replicate after replicate, ``np.bincount(rng.integers(0, L, size=L), minlength=L)``."""
    L, B = int(L), int(B)
    if L < 1 or B < 0:
        raise ValueError(f"bootstrap_multiplicities: {L} columns, {B} replicates")
    rng = np.random.default_rng(seed)
    out = np.zeros((B, L), dtype=np.int32)
    for b in range(B):
        out[b] = np.bincount(rng.integers(0, L, size=L), minlength=L)
    return out


def nj_tree(snp_dat=None, *, dist=None, labels=None, engine=None, alignment_resident=False, clamp_negative=True, per_site=False, bootstrap=0, seed=0,
            multiplicities=None) -> Tree:
    """The neighbour-joining tree, built on the device, of ``snp_dat``'s sequences under the Hamming distance of the five-state rule (the number of
    SNP columns at which two sequences differ: what ``estimate_Hamming_distance_weights`` thresholds), or of ``dist``, a symmetric (n, n) float64
    matrix with a zero diagonal.  ``engine`` with ``alignment_resident=True``: the engine already holds the alignment (``snp_dat`` may then be None).
    Tips are labelled ``labels``, else ``snp_dat.seq_names``, else 1 .. n, in sequence order.  The tree is unrooted: its root is the trifurcation of
    the last three nodes, children in ascending node id (a join's: smaller id, larger id); ``midpoint_root`` roots it.  ``clamp_negative``: see
    ``nj_clamp`` (``midpoint_root`` rejects negative branches).  ``per_site`` divides the lengths by the number of SNP columns.  Needs a GPU.

    ``bootstrap=B`` (B > 0) adds bootstrap support, computed on the device (``Engine.nj_bootstrap``): B replicates drawn by
    ``bootstrap_multiplicities(L, B, seed)``, or the rows of ``multiplicities``, an int (B, L) array of column multiplicities 0..63 of your own.  The
    tree then has ``support`` — per node the number of replicates whose tree has the branch above it, -1 at the tips and the root — and
    ``n_replicates``.  A matrix has no columns to resample: with ``dist`` either argument raises ValueError."""
    from .engine import Engine
    if bootstrap < 0:
        raise ValueError("nj_tree: bootstrap must be >= 0")
    want_support = bootstrap > 0 or multiplicities is not None
    if dist is not None and want_support:
        raise ValueError("nj_tree: bootstrap support needs an alignment: a distance matrix has no columns to resample")
    if dist is not None and (snp_dat is not None or alignment_resident):
        raise ValueError("nj_tree: pass either dist or an alignment")
    if dist is None and snp_dat is None and not alignment_resident:
        raise ValueError("nj_tree: nothing to build a tree of: pass snp_dat, dist, or an engine with alignment_resident=True")
    if alignment_resident and engine is None:
        raise ValueError("alignment_resident=True needs the engine that holds the alignment")
    if dist is not None and per_site:
        raise ValueError("nj_tree: per_site needs an alignment")
    own = engine is None
    eng = Engine(0) if own else engine
    support, n_rep = None, None
    try:
        if dist is not None:
            parent, length = eng.nj_tree(dist)
        else:
            if not alignment_resident:
                if snp_dat.states is None:
                    raise ValueError("snp_dat.states is None (the alignment stayed on the device): pass its engine with alignment_resident=True")
                eng.set_alignment(snp_dat.states)
            n_snp = eng.L
            if want_support:
                mult = bootstrap_multiplicities(n_snp, bootstrap, seed) if multiplicities is None else np.asarray(multiplicities)
                if mult.ndim != 2 or (bootstrap and mult.shape[0] != bootstrap):
                    raise ValueError(f"nj_tree: multiplicities of shape {mult.shape} for bootstrap = {bootstrap}")
                parent, length, support = eng.nj_bootstrap(mult)
                n_rep = int(mult.shape[0])
            else:
                parent, length = eng.nj_tree()
    finally:
        if own:
            eng.close()
    if labels is None:
        names = list(getattr(snp_dat, "seq_names", None) or [])
        labels = names if 2 * len(names) - 2 == len(parent) else None
    if per_site:
        length = length / float(n_snp)
    return tree_from_joins(parent, length, labels, clamp_negative, support, n_rep)


def tree_from_joins(parent, length, labels=None, clamp_negative=True, support=None, n_replicates=None) -> Tree:
    """The ``Tree`` of ``Engine.nj_tree``'s (parent, length): the root is node 2n - 3, the children of every node in ascending node id, the tips
    labelled ``labels`` (default 1 .. n) in node order.  ``support``, where given, is ``Engine.nj_bootstrap``'s, per node of the joins."""
    parent, length = np.asarray(parent), np.asarray(length, dtype=np.float64)
    n = (len(parent) + 2) // 2
    labels = [str(k + 1) for k in range(n)] if labels is None else [str(x) for x in labels]
    if len(labels) != n:
        raise ValueError(f"{len(labels)} labels for {n} tips")
    if clamp_negative:
        length = nj_clamp(parent, length)
    root = 2 * n - 3
    kids = [[] for _ in range(2 * n - 2)]
    for v in range(root):
        kids[int(parent[v])].append(v)
    ln = length.tolist()
    sup = None if support is None else np.asarray(support).tolist()
    return _build(root, lambda v: kids[v], lambda v: ln[v], lambda v: v if v < n else -1, labels, None if sup is None else (lambda v: sup[v]), n_replicates)


# ---- rooting and ordering ---------------------------------------------------------------------------------------------------------------------------

def _dist_from(tree: Tree, s: int) -> list:
    """Path lengths from node s to every node: up the ancestors of s, then down every other branch (a parent has the smaller number)."""
    par, ln = tree.parent.tolist(), tree.length.tolist()
    d = [-1.0] * tree.n_nodes
    d[s] = 0.0
    v = s
    while par[v] >= 0:
        d[par[v]] = d[v] + ln[v]
        v = par[v]
    for v in range(1, tree.n_nodes):
        if d[v] < 0.0:
            d[v] = d[par[v]] + ln[v]
    return d


def diameter_tips(tree: Tree):
    """(a, b, distances from a to every node): a = the tip farthest from tip 0, b = the tip farthest from a; ties go to the lowest tip index."""
    tips = tree.tip_node
    d0 = np.asarray(_dist_from(tree, int(tips[0])))
    a = int(np.argmax(d0[tips]))
    da = _dist_from(tree, int(tips[a]))
    return a, int(np.argmax(np.asarray(da)[tips])), da


def midpoint_root(tree: Tree) -> Tree:
    """The tree rooted half way between its two most distant tips, in O(nodes): a = the tip farthest from tip 0, b = the tip farthest from a (ties:
    the lowest tip index of the file); the root lies on the path from a to b at half their distance from a.  Where that point is a node, the node
    becomes the root; otherwise its branch is split.  An old root left with two branches is removed and their lengths are added.  A node that
    changes direction gets its old parent as its last child.  Negative lengths and a tree whose lengths are all zero raise ValueError.  ``support``
    stays with its branch: both halves of a split branch keep the branch's, and the one branch made of the removed old root's two takes the larger."""
    ln = tree.length
    if np.any(ln[1:] < 0) or np.any(~np.isfinite(ln[1:])):
        raise ValueError("midpoint_root: the tree has a negative or non-finite branch length")
    if not np.any(ln[1:] > 0):
        raise ValueError("midpoint_root: every branch length is zero")
    tips = tree.tip_node
    a, b, da = diameter_tips(tree)
    half = da[int(tips[b])] / 2.0
    par = tree.parent.tolist()
    # the path from a to b: up from a to the common ancestor, down to b
    up_a, v = [], int(tips[a])
    while v >= 0:
        up_a.append(v)
        v = par[v]
    on_a = {v: k for k, v in enumerate(up_a)}
    down_b, v = [], int(tips[b])
    while v not in on_a:
        down_b.append(v)
        v = par[v]
    path = up_a[:on_a[v] + 1] + down_b[::-1]
    k = next(k for k, v in enumerate(path) if da[v] >= half)
    n_old = tree.n_nodes
    lnl = ln.tolist()
    if da[path[k]] == half:
        new_root, split = path[k], None
    else:
        u, w = path[k - 1], path[k]
        c = u if par[u] == w else w              # the lower end of the split branch
        p = par[c]
        new_root, split = n_old, (c, p)
        len_c = half - da[u] if c == u else da[w] - half
        len_p = lnl[c] - len_c

    def nbrs(v):
        if v == n_old:
            return [split[0], split[1]]
        out = tree.children(v).tolist()
        if par[v] >= 0:
            out.append(par[v])
        if split and v in split:
            out = [n_old if (x == split[1] and v == split[0]) or (x == split[0] and v == split[1]) else x for x in out]
        return out

    def edge(v, u):
        if split and n_old in (v, u):
            return len_c if split[0] in (v, u) else len_p
        return lnl[v] if par[v] == u else lnl[u]

    supl = None if tree.support is None else tree.support.tolist()

    def esup(v, u):                              # support belongs to the branch, whichever way it now points; both halves of the split branch keep it
        if supl is None:
            return -1
        if split and n_old in (v, u):
            return supl[split[0]]
        return supl[v] if par[v] == u else supl[u]

    kids, up, stack = {}, {new_root: (-1, 0.0, -1)}, [new_root]
    while stack:
        v = stack.pop()
        kids[v] = [u for u in nbrs(v) if u != up[v][0]]
        for u in kids[v]:
            up[u] = (v, edge(v, u), esup(v, u))
            stack.append(u)
    old = 0
    if old != new_root and len(kids[old]) <= 1:  # the old root is left with two branches (or, a root of one child, with one): it goes
        q, l_up, s_up = up[old]
        if kids[old]:
            only = kids[old][0]
            up[only] = (q, up[only][1] + l_up, max(up[only][2], s_up))   # one branch of the two: the larger support
            kids[q] = [only if x == old else x for x in kids[q]]
        else:
            kids[q] = [x for x in kids[q] if x != old]
    tip_of = {int(v): t for t, v in enumerate(tips.tolist())}
    return _build(new_root, lambda v: kids[v], lambda v: up[v][1], lambda v: tip_of.get(v, -1), tree.tip_label,
                  None if supl is None else (lambda v: up[v][2]), tree.n_replicates)


def ladderize(tree: Tree) -> Tree:
    """Children ordered by ascending number of tips below them, ties in the order they had."""
    n = tree.n_nodes
    cnt = np.zeros(n, dtype=np.int64)
    cnt[tree.tip_node] = 1
    par = tree.parent.tolist()
    c = cnt.tolist()
    for v in range(n - 1, 0, -1):
        c[par[v]] += c[v]
    tip_of = {int(v): t for t, v in enumerate(tree.tip_node.tolist())}
    lnl = tree.length.tolist()
    supl = None if tree.support is None else tree.support.tolist()
    return _build(0, lambda v: sorted(tree.children(v).tolist(), key=lambda u: c[u]), lambda v: lnl[v], lambda v: tip_of.get(v, -1), tree.tip_label,
                  None if supl is None else (lambda v: supl[v]), tree.n_replicates)


# ---- the reference's selection (R/preptrees.R:67-179) ---------------------------------------------------------------------------------------------------

def _r_seq(n):
    """The 1-based indices ``1:n`` as a subscript: 1..floor(n), and for n < 1 R's descending 1, 0, of which the 0 selects nothing."""
    n = int(math.floor(n))
    return list(range(1, n + 1)) if n >= 1 else [1]


def _fmt_pos(x) -> str:
    x = float(x)
    return str(int(x)) if x.is_integer() else repr(x)


def _read_links(path, sr: bool, what: str):
    from .output import read_TopHits
    df = read_TopHits(os.path.realpath(path))
    if sr:       # :75-76, :80-81
        hit = [c for c in df.columns if str(c).lower() == "srp"]
        if len(hit) != 1:
            raise ValueError(f"{what} file does not contain the srp column!")
        df = df.drop(columns=hit)
    return df


def _rbind(frames, what):
    import pandas as pd
    frames = [f for f in frames if f is not None]
    if not frames:
        return None
    for f in frames[1:]:
        if list(f.columns) != list(frames[0].columns) and sorted(map(str, f.columns)) != sorted(map(str, frames[0].columns)):
            raise ValueError(f"view_tree: the {what} tables have different columns: {list(frames[0].columns)} and {list(f.columns)}")
    return pd.concat([f[list(frames[0].columns)] for f in frames], ignore_index=True)


def tree_links(links_df=None, lr_tophits_path=None, lr_annotated_links_path=None, sr_tophits_path=None, sr_annotated_links_path=None):
    """``top_hits`` of :67-87: ``links_df`` as given, or the four link files — ``srp`` dropped from the short-range ones, each range's rows bound,
    whole-row duplicates removed (the first stays), tagged ``link`` = sr / lr, short-range rows first.  None without any input."""
    if links_df is not None:
        return links_df.reset_index(drop=True)
    lrt = _read_links(lr_tophits_path, False, "lr_tophits") if lr_tophits_path is not None else None
    lra = _read_links(lr_annotated_links_path, False, "lr_annotated_links") if lr_annotated_links_path is not None else None
    srt = _read_links(sr_tophits_path, True, "sr_tophits") if sr_tophits_path is not None else None
    sra = _read_links(sr_annotated_links_path, True, "sr_annotated_links") if sr_annotated_links_path is not None else None
    parts = []
    for frames, tag in (((srt, sra), "sr"), ((lrt, lra), "lr")):
        t = _rbind(frames, tag)
        if t is not None:
            t = t[~t.duplicated()].reset_index(drop=True)
            t["link"] = tag
            parts.append(t)
    return _rbind(parts, "sr and lr")


def tree_columns(top_hits, pos, have_links_df: bool, ntop_links=10, from_=None, to=None):
    """:99-161 without the FASTA: (``pos_plot``, the kept positions ascending, and for each its 0-based line of the pos file).  A position that matches
    not exactly one line of the pos file is dropped with the reference's warning."""
    if from_ is not None and to is None:
        raise ValueError("<to> must also be provided")
    if to is not None and from_ is None:
        raise ValueError("<from> must also be provided")
    if from_ is not None:
        if to < from_:
            raise ValueError("<from> must be less than <to>")
        if from_ < 0:
            raise ValueError("<from> must be positive")
        from_, to = round(from_), round(to)
        ntop_links = None
    if ntop_links is not None:
        if ntop_links < 0:
            raise ValueError("<ntop_links> must be positive")
        if ntop_links > 10:
            warnings.warn("Plot may be cluttered due to large <ntop_links> value")
    n = 0 if top_hits is None else len(top_hits)
    chosen = []
    if ntop_links is not None and n:
        if have_links_df:        # (the reference tests links_df after rm(links_df): an error in R; its documentation says the first ntop_links rows)
            chosen += [k for k in _r_seq(ntop_links) if k <= n]
        else:
            link = list(top_hits["link"])
            for tag in ("lr", "sr"):     # :125-128
                rows = [k + 1 for k in range(n) if link[k] == tag]
                chosen += [rows[k - 1] for k in _r_seq(ntop_links) if k <= len(rows)]
    p1 = [] if top_hits is None else [float(v) for v in top_hits["pos1"]]
    p2 = [] if top_hits is None else [float(v) for v in top_hits["pos2"]]
    if from_ is not None:        # :132-136
        chosen = list(dict.fromkeys([k + 1 for k in range(n) if from_ <= p1[k] <= to] + [k + 1 for k in range(n) if from_ <= p2[k] <= to]))
    pos_plot, cols = [], []
    if chosen:
        cand = sorted({v for v in [p1[k - 1] for k in chosen] + [p2[k - 1] for k in chosen] if v == v})     # :140 (sort drops NA)
        pos = [float(v) for v in pos]
        for v in cand:           # :143-151
            idx = [j for j, q in enumerate(pos) if q == v]
            if len(idx) != 1:
                warnings.warn(f"{_fmt_pos(v)} not available in the provided fasta file(s)")
                continue
            pos_plot.append(v)
            cols.append(idx[0])
    return pos_plot, cols


def read_pos_file(path):
    """``as.numeric(readLines(pos_file_path))``."""
    out = []
    with open(path, "r") as fh:
        for ln in fh.read().splitlines():
            try:
                out.append(float(ln.strip()))
            except ValueError:
                out.append(float("nan"))
    return out


def tree_fasta(fasta_path, n_pos: int, tip_label):
    """``read_fasta`` (:217-239): the character matrix uint8 [tips, n_pos] with its rows in tip order; every tip label must match exactly one sequence
    name, other sequences are allowed.  Characters stay as the file has them (no case folding)."""
    from .snpdat import read_fasta
    names, chars = read_fasta(fasta_path)
    if chars.shape[1] != n_pos:      # (the reference: .readFasta answers seq.length = -1 and the matrix construction fails)
        raise ValueError(f"the sequences of {fasta_path} have {chars.shape[1]} characters but the position file has {n_pos} lines")
    where = {}
    for k, s in enumerate(names):
        where.setdefault(s, []).append(k)
    rows = []
    for t in tip_label:
        if len(where.get(t, ())) != 1:
            raise ValueError("Sequence names mismatch between provided tree file and fasta file")
        rows.append(where[t][0])
    return chars[np.asarray(rows, dtype=np.int64)]


def metadata_id_column(metadata_df) -> int:
    hit = [k for k, c in enumerate(metadata_df.columns) if str(c).lower() == "id"]     # :94-95
    if len(hit) != 1:
        raise ValueError("Metadata file must contain an ID column")
    return hit[0]


def tree_metadata(metadata_df, tip_label):
    """:165-179: (column names without the id column, values [tips][columns] with the rows in tip order; the first row of a repeated id)."""
    idc = metadata_id_column(metadata_df)
    ids = [str(v) for v in metadata_df.iloc[:, idc]]
    first = {}
    for k, s in enumerate(ids):
        first.setdefault(s, k)
    rows = []
    for t in tip_label:
        if t not in first:
            raise ValueError("Entry in tree$tip.label missing in <metadata_df> ids")
        rows.append(first[t])
    cols = [k for k in range(metadata_df.shape[1]) if k != idc]
    names = [str(metadata_df.columns[k]) for k in cols]
    vals = [[metadata_df.iat[r, k] for k in cols] for r in rows]
    return names, vals


def tree_selection(tip_label, metadata_df=None, fasta_path=None, pos_file_path=None, links_df=None, lr_tophits_path=None, lr_annotated_links_path=None,
                   sr_tophits_path=None, sr_annotated_links_path=None, ntop_links=10, from_=None, to=None) -> dict:
    """:67-179 in the reference's order, on the host: ``pos_plot`` and ``cols`` (``tree_columns``), ``chars`` (``tree_fasta``), ``metadata_columns`` and
    ``metadata_values`` (``tree_metadata``)."""
    if fasta_path is None or pos_file_path is None:
        raise ValueError("fasta_path and pos_file_path must be provided")
    top_hits = tree_links(links_df, lr_tophits_path, lr_annotated_links_path, sr_tophits_path, sr_annotated_links_path)
    pos = read_pos_file(pos_file_path)                       # :90-91
    chars = tree_fasta(fasta_path, len(pos), tip_label)
    if metadata_df is not None:
        metadata_id_column(metadata_df)
    pos_plot, cols = tree_columns(top_hits, pos, links_df is not None, ntop_links, from_, to)
    names, vals = tree_metadata(metadata_df, tip_label) if metadata_df is not None else ([], [])
    return dict(pos_plot=pos_plot, cols=cols, chars=chars, metadata_columns=names, metadata_values=vals)


def _meta_value(v):
    """A metadata cell as the string the levels are made of; None for a missing one (None, NaN, NA)."""
    import pandas as pd
    return None if v is None or bool(pd.isna(v)) else str(v)


def group_levels(rows):
    """The levels of a group of bands: ``rows`` [bands][tips] of values of one kind (character codes, or strings; None: missing) to (uint8 [bands,
    tips], the distinct values in code-point order).  Level k of n is drawn in ``hue_palette(n)[k]``; missing is level 255."""
    keyed = rows
    vals = sorted({v for r in keyed for v in r if v is not None})
    if len(vals) > MISSING_LEVEL:
        raise ValueError(f"{len(vals)} distinct values in one group of bands (at most {MISSING_LEVEL})")
    code = {v: k for k, v in enumerate(vals)}
    lev = np.asarray([[MISSING_LEVEL if v is None else code[v] for v in r] for r in keyed], dtype=np.uint8).reshape(len(rows), -1)
    return lev, vals


def group_palette(n_levels: int) -> np.ndarray:
    pal = np.full(256, MISSING_RGB, dtype=np.uint32)
    pal[:n_levels] = hue_palette(n_levels) if n_levels else []
    return pal


# ---- the layout -------------------------------------------------------------------------------------------------------------------------------------------

def _half_up(v) -> int:
    return int(math.floor(v + 0.5))


def text_scale(width: int) -> int:
    return max(1, _half_up(width / 1500.0))


def _text_width(s: str, sc: int) -> int:
    n = len(s.encode("utf-8", "replace"))
    return n * 6 * sc - sc if n else 0


def tree_layout(tree: Tree, width: int, height: int, n_metadata: int = 0, n_alleles: int = 0, offset_metadata=None, offset_alleles=None, width_metadata=None,
                width_alleles=None, band_labels=(), legends=(), thickness: int = 16, support_min=None, n_replicates=None) -> dict:
    """Every rectangle of the figure (x, y, w, h in canvas pixels) and the bars of the tree.  Root at the top.  The margins: 20 text-scale pixels on top
    (the title), 4 below; left, room for the longest band label (at least width / 20); right, room for the widest legend (at least width / 10).  The tree
    panel is T pixels high, T = floor(available height / (1 + E)), E the larger lower end of the two groups of bands: the offsets and widths are
    fractions of T measured from the tip line, which is the panel's lower edge, as ggtree's gheatmap measures them from the tips (defaults of the
    reference, K = allele columns: width_metadata K / 200, offset_metadata 0, offset_alleles K / 100, width_alleles 5).  Band r of n in a group
    spans the pixel rows floor(T (offset + r width / n)) .. floor(T (offset + (r + 1) width / n)) below the tip line; an empty band and overlapping
    groups raise ValueError.  Tip slot i of N (figure order) spans [i, i + 1) PW / N of the panel; a tip's x is the middle of its slot, a node's the
    midpoint of its first and last child; y = 0.5 + depth / max depth (T - 1) pixels; both rounded half up to 1/16 pixel.  Bars (1/16 pixel, relative
    to the panel): per branch [x - t/2, x + t/2) x [y parent, y), per internal node the connector [x first - t/2, x last + t/2) x [y - t/2, y + t/2).
    With ``support_min`` and ``n_replicates`` and a tree that has ``support``, every internal node whose support is >= support_min x n_replicates is
    marked by a knob: a square of side 3 t centred on the node, one more bar each, appended after the bars above in node order.
    Returns a dict: canvas, panel, bands (metadata then alleles), legend_xy, text_scale, bars, tip_order, node_x / node_y (1/16 pixel), support_nodes
    (int32: the marked nodes)."""
    K = n_alleles
    if width_metadata is None:
        width_metadata = K / 200.0      # :183-186
    if offset_metadata is None:
        offset_metadata = 0.0
    if offset_alleles is None:
        offset_alleles = K / 100.0
    if width_alleles is None:
        width_alleles = 5.0
    W, H = int(width), int(height)
    if not (1 <= W <= MAX_CANVAS and 1 <= H <= MAX_CANVAS):
        raise ValueError(f"a canvas of {W} x {H} pixels (1..{MAX_CANVAS} each way)")
    sc = text_scale(W)
    th, gap = 7 * sc, 2 * sc
    top, bottom = 20 * sc, 4 * sc
    left = max(W // 20, max([_text_width(s, sc) for s in band_labels], default=0) + 3 * gap)
    leg_w = 0
    for title, labels, _ in legends:
        if labels:
            leg_w = max(leg_w, _text_width(title, sc), th + gap + max(_text_width(s, sc) for s in labels))
    right = max(W // 10, leg_w + 4 * gap)
    PW = W - left - right
    groups = [(n_metadata, float(offset_metadata), float(width_metadata), "metadata"), (n_alleles, float(offset_alleles), float(width_alleles), "alleles")]
    ext = 0.0
    for n, off, wd, what in groups:
        if n:
            if not (off >= 0 and wd > 0 and math.isfinite(off) and math.isfinite(wd)):
                raise ValueError(f"offset_{what} must be >= 0 and width_{what} > 0")
            ext = max(ext, off + wd)
    T = int(math.floor((H - top - bottom) / (1.0 + ext)))
    if PW < 1 or T < 2:
        raise ValueError(f"a canvas of {W} x {H} pixels leaves no room for the tree panel")
    tip_y = top + T
    bands, spans = [], []
    for n, off, wd, what in groups:
        if not n:
            continue
        for r in range(n):
            y0, y1 = int(math.floor(T * (off + r * wd / n))), int(math.floor(T * (off + (r + 1) * wd / n)))
            if y1 <= y0:
                raise ValueError(f"{what} band {r} has no pixel row: raise width_{what} or the plot height")
            bands.append((left, tip_y + y0, PW, y1 - y0))
        spans.append((bands[-n][1], bands[-1][1] + bands[-1][3], what))
    if len(spans) == 2 and spans[0][0] < spans[1][1] and spans[1][0] < spans[0][1]:
        raise ValueError("the metadata bands and the allele bands overlap: change the offsets or widths")
    for x, y, w, h in bands:
        if y + h > H:
            raise ValueError("a band leaves the canvas")      # (not reached: T is sized for the bands)
    # the legends, one under the other in the right margin
    legend_xy, y = [], top
    for title, labels, _ in legends:
        legend_xy.append((W - right + 2 * gap, y))
        if labels:
            y += (len(labels) + 1) * (th + gap) + 2 * gap
    # the tree
    N, n_nodes = tree.n_tips, tree.n_nodes
    order = tree.tip_order()
    x = [0.0] * n_nodes
    tn = tree.tip_node.tolist()
    for slot, t in enumerate(order.tolist()):
        x[tn[t]] = (slot + 0.5) * PW / N
    ptr, idx = tree.child_ptr.tolist(), tree.child_idx.tolist()
    for v in range(n_nodes - 1, -1, -1):
        if ptr[v + 1] > ptr[v]:
            x[v] = (x[idx[ptr[v]]] + x[idx[ptr[v + 1] - 1]]) / 2.0
    depth = tree.depths()
    dmax = float(depth.max())
    X = [_half_up(v * 16.0) for v in x]
    Y = [_half_up((0.5 + (d / dmax if dmax > 0 else 0.0) * (T - 1)) * 16.0) for d in depth.tolist()]
    par = tree.parent.tolist()
    h0, h1 = thickness // 2, thickness - thickness // 2
    bars = []
    for v in range(n_nodes):
        if v and Y[v] > Y[par[v]]:
            bars.append((X[v] - h0, Y[par[v]], X[v] + h1, Y[v]))
        if ptr[v + 1] > ptr[v]:
            bars.append((X[idx[ptr[v]]] - h0, Y[v] - h0, X[idx[ptr[v + 1] - 1]] + h1, Y[v] + h1))
    marked = []
    if tree.support is not None and support_min is not None and n_replicates:
        need, sup = float(support_min) * float(n_replicates), tree.support.tolist()
        marked = [v for v in range(n_nodes) if ptr[v + 1] > ptr[v] and sup[v] >= 0 and sup[v] >= need]
        k0, k1 = (3 * thickness) // 2, 3 * thickness - (3 * thickness) // 2
        bars += [(X[v] - k0, Y[v] - k0, X[v] + k1, Y[v] + k1) for v in marked]
    from .engine import Engine
    barr = np.zeros(len(bars), dtype=Engine.BAR)
    if bars:
        b = np.asarray(bars, dtype=np.int32)
        barr["x0"], barr["y0"], barr["x1"], barr["y1"] = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    return dict(canvas=(W, H), panel=(left, top, PW, T), bands=np.asarray(bands, dtype=np.int32).reshape(-1, 4), legend_xy=legend_xy, text_scale=sc,
                bars=barr, tip_order=order, node_x=np.asarray(X, dtype=np.int32), node_y=np.asarray(Y, dtype=np.int32),
                support_nodes=np.asarray(marked, dtype=np.int32))


# ---- view_tree ------------------------------------------------------------------------------------------------------------------------------------------------

def view_tree(tree_path=None, perform_midpoint_rooting=True, metadata_df=None, fasta_path=None, pos_file_path=None, links_df=None, lr_tophits_path=None,
              lr_annotated_links_path=None, sr_tophits_path=None, sr_annotated_links_path=None, ntop_links=10, from_=None, to=None, offset_metadata=None,
              offset_alleles=None, width_metadata=None, width_alleles=None, plot_save_path=None, plot_height=20, plot_width=15, *, engine=None,
              want_canvas=False, dpi=300, bootstrap=0, seed=0, support_min=0.7):
    """``view_tree`` (R/preptrees.R:45-215; ``from`` is spelled ``from_``).  The canvas has plot_width dpi x plot_height dpi pixels, at most 8192
    either way.  Returns a dict: ``tree`` (rooted and ladderized), ``tip_order``, ``pos_plot`` (the allele columns), ``metadata_columns``, ``alleles``
    / ``metadata`` (levels uint8 [bands, tips in figure order] and their values), ``layout`` (``tree_layout``), ``boxes`` (what the host drew: band
    labels, title, two legends), ``png`` (the path written, or None) and ``canvas`` (uint8 [H, W, 3]: with ``want_canvas`` or without a path, when no
    file is written).  The figure needs a GPU.

    Without ``tree_path`` the tree is built from the sequences of ``fasta_path``: encoded by the five-state rule, joined by ``nj_tree`` on an engine of
    its own (the caller's keeps its alignment), the tips named as the FASTA names them, in file order; the figure's title is then ``NJ (Hamming)``.

    ``bootstrap=B`` (B > 0): the built tree gets the support of B bootstrap replicates (``nj_tree(bootstrap=B, seed=seed)``), the title becomes
    ``NJ (Hamming), B = <B>`` and every internal node whose support is >= ``support_min`` x B is marked by a square knob (``tree_layout``;
    ``layout["support_nodes"]``).  With ``tree_path``, B is the number of replicates the file's integer internal labels count: the same marks."""
    if fasta_path is None or pos_file_path is None:
        raise ValueError("fasta_path and pos_file_path must be provided")
    if bootstrap < 0:
        raise ValueError("bootstrap must be >= 0")
    W, H = _half_up(float(plot_width) * dpi), _half_up(float(plot_height) * dpi)
    if not (1 <= W <= MAX_CANVAS and 1 <= H <= MAX_CANVAS):
        raise ValueError(f"the canvas of {W} x {H} pixels (plot_width x dpi by plot_height x dpi) must lie in 1..{MAX_CANVAS} either way")
    if tree_path is None:
        from .snpdat import SnpDat, encode_chars, read_fasta
        names, seq = read_fasta(fasta_path)
        states = np.ascontiguousarray(encode_chars(seq).T)
        tree = nj_tree(SnpDat(states=states, POS=np.arange(states.shape[0], dtype=np.int32), g=None, uqe=None, r=None, seq_names=names), labels=names,
                       bootstrap=bootstrap, seed=seed)
        # through its Newick text, so that the figure is the one ``view_tree`` draws of the written tree: a file numbers its tips in its own
        # order, and midpoint rooting breaks its ties by tip number
        tree = parse_newick(write_newick(tree).encode("utf-8", "surrogateescape"))
        title = f"NJ (Hamming), B = {bootstrap}" if bootstrap else "NJ (Hamming)"
    else:
        tree = read_newick(os.path.realpath(tree_path))      # :64-65
        title = os.path.basename(str(tree_path))
    if bootstrap and tree.support is not None:
        tree.n_replicates = int(bootstrap)                   # (Newick text carries the counts, not what they are counts of)
    if perform_midpoint_rooting:
        tree = midpoint_root(tree)
    sel = tree_selection(tree.tip_label, metadata_df, fasta_path, pos_file_path, links_df, lr_tophits_path, lr_annotated_links_path, sr_tophits_path,
                         sr_annotated_links_path, ntop_links, from_, to)
    pos_plot, cols, chars, meta_names, meta_vals = sel["pos_plot"], sel["cols"], sel["chars"], sel["metadata_columns"], sel["metadata_values"]
    tree = ladderize(tree)                                   # :181
    order = tree.tip_order()
    al_lev, al_vals = group_levels([[int(chars[t, c]) for t in order] for c in cols]) if cols else (np.zeros((0, tree.n_tips), dtype=np.uint8), [])
    md_lev, md_vals = (group_levels([[_meta_value(meta_vals[t][k]) for t in order] for k in range(len(meta_names))]) if meta_names
                       else (np.zeros((0, tree.n_tips), dtype=np.uint8), []))
    labels = meta_names + [_fmt_pos(v) for v in pos_plot]
    md_pal, al_pal = group_palette(len(md_vals)), group_palette(len(al_vals))
    md_missing, al_missing = bool(np.any(md_lev == MISSING_LEVEL)), False
    legends = [("Metadata", [str(v) for v in md_vals] + (["NA"] if md_missing else []), [int(v) for v in md_pal[:len(md_vals)]] + ([MISSING_RGB] if md_missing else [])),
               ("Alleles", [chr(v) for v in al_vals], [int(v) for v in al_pal[:len(al_vals)]])]
    lay = tree_layout(tree, W, H, len(meta_names), len(cols), offset_metadata, offset_alleles, width_metadata, width_alleles, labels, legends,
                      support_min=support_min if bootstrap else None, n_replicates=bootstrap or None)
    levels = np.concatenate([md_lev, al_lev], axis=0)
    palette = np.stack([md_pal] * len(md_lev) + [al_pal] * len(al_lev)) if len(levels) else np.zeros((0, 256), dtype=np.uint32)
    from .engine import Engine
    own = engine is None
    eng = Engine(0) if own else engine
    need_canvas = want_canvas or plot_save_path is None
    try:
        canvas, boxes = eng.plot_tree(W, H, lay["panel"], lay["bars"], TREE_RGB, levels, palette, lay["bands"], labels, title,
                                      [(t, l, c, xy) for (t, l, c), xy in zip(legends, lay["legend_xy"])], lay["text_scale"], png_path=plot_save_path,
                                      want_canvas=need_canvas)
    finally:
        if own:
            eng.close()
    return dict(tree=tree, tip_order=order, pos_plot=pos_plot, metadata_columns=meta_names, alleles=(al_lev, al_vals), metadata=(md_lev, md_vals), levels=levels,
                palette=palette, layout=lay, boxes=boxes, png=None if plot_save_path is None else str(plot_save_path), canvas=canvas)
