"""numpy restatement of the lineage check: single-linkage clusters of the sequences from the shared-state counts, and per cluster the
joint tables and the weighted MI of listed SNP pairs.  The kernels (csrc/ldw_lineage.hip), this file and the tests follow include/ldweaver_amd.h (18)."""
from __future__ import annotations

import math

import numpy as np


# ---- clusters -------------------------------------------------------------------------------------------------------------------------------------
def adjacency(states: np.ndarray, thresh: int) -> np.ndarray:
    """bool (N, N): i and j are neighbours iff L - shared(i, j) < thresh (the predicate of the Hamming weights; the diagonal included)."""
    L, N = states.shape
    shared = np.zeros((N, N), dtype=np.int64)
    for x in range(5):
        m = (states == x).astype(np.float64)
        shared += np.rint(m.T @ m).astype(np.int64)
    return (L - shared) < int(thresh)


def canonical(root: np.ndarray):
    """Labels 0, 1, ... in the order of the clusters' smallest members, from any array that is constant on a cluster and differs between clusters."""
    root = np.asarray(root)
    _, first, inv = np.unique(root, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inv.ravel()].astype(np.int32), int(len(first))


def components_union_find(adj: np.ndarray):
    """(labels int32 [N], n_clusters): connected components by union-find over the edges, canonically numbered."""
    N = adj.shape[0]
    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, j in zip(*np.nonzero(np.triu(adj, 1))):
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)
    return canonical(np.asarray([find(x) for x in range(N)]))


def components_bfs(adj: np.ndarray):
    """The same by a breadth-first search from every unvisited vertex in ascending order."""
    N = adj.shape[0]
    lab = np.full(N, -1, dtype=np.int32)
    n = 0
    for s in range(N):
        if lab[s] >= 0:
            continue
        lab[s] = n
        front = [s]
        while front:
            nxt = []
            for u in front:
                for v in np.nonzero(adj[u])[0].tolist():
                    if lab[v] < 0:
                        lab[v] = n
                        nxt.append(v)
            front = nxt
        n += 1
    return lab, n


def components_hook_jump(adj: np.ndarray, jumps: int = 2):
    """(labels, n_clusters, rounds): the synchronous statement of the device's rounds.  f[u] starts at u.  A round: m[u] = the smallest f over u's
    neighbours; where m[u] < f[u], f[f[u]] and f[u] are lowered to m[u] (hook onto the root, then the vertex itself); then ``jumps`` times f = f[f].
    The rounds end with the first one that changes nothing; f[u] is then the smallest member of u's cluster."""
    N = adj.shape[0]
    a = adj.copy()
    np.fill_diagonal(a, False)
    f = np.arange(N, dtype=np.int64)
    big = np.iinfo(np.int64).max
    rounds = 0
    while True:
        rounds += 1
        old = f.copy()
        m = np.where(a, old[None, :], big).min(axis=1) if N else old
        hook = m < old
        np.minimum.at(f, old[hook], m[hook])
        np.minimum.at(f, np.nonzero(hook)[0], m[hook])
        for _ in range(jumps):
            f = f[f]
        if np.array_equal(f, old):
            break
    lab, n = canonical(f)
    return lab, n, rounds


def seq_clusters(states: np.ndarray, thresh):
    """(labels int32 (n_thresh, N), n_clusters int32 (n_thresh,)) as ldw_seq_clusters states them."""
    th = np.atleast_1d(np.asarray(thresh, dtype=np.int64))
    out = [components_union_find(adjacency(states, int(t))) for t in th]
    return np.stack([o[0] for o in out]), np.asarray([o[1] for o in out], dtype=np.int32)


# ---- stratified tables and MI -----------------------------------------------------------------------------------------------------------------------
def quantise(hdw: np.ndarray):
    """(V int64 [N], F): ldw_set_weights' fixed point, V_s = round(fl(sqrt w)^2 2^F) in five balanced base-256 digits, every sum below 2^52."""
    hdw = np.asarray(hdw, dtype=np.float64)
    sq = np.sqrt(hdw)
    v = sq * sq
    if np.all(v == 1.0):
        return np.ones(len(v), dtype=np.int64), 0
    lim_digits = 0.99 * math.ldexp(1.0, 39) / float(v.max())
    lim_sum = math.ldexp(1.0, 52) / float(np.sum(v.astype(np.longdouble)))
    F = int(math.floor(math.log2(min(lim_digits, lim_sum))))
    return np.rint(np.ldexp(v, F)).astype(np.int64), F


def mi_from_tables(counts: np.ndarray, fixed: np.ndarray, F: int, neff: float) -> float:
    """The formula of include/ldweaver_amd.h (18) on one cluster's 5 x 5 integer tables."""
    counts, fixed = np.asarray(counts).reshape(5, 5), np.asarray(fixed).reshape(5, 5)
    pa, pb = counts.sum(axis=1) > 0, counts.sum(axis=0) > 0
    ra, rb = float(pa.sum()), float(pb.sum())
    if ra <= 1 and rb <= 1:             # no member, or both SNPs monomorphic: the formula's log 1, not left to rounding
        return 0.0
    scale = math.ldexp(1.0, -F)
    den = neff + 0.5 * ra * rb
    mi = 0.0
    for X in range(5):
        if not pa[X]:
            continue
        pX = float(int(fixed[X].sum())) * scale
        for Y in range(5):
            if not pb[Y]:
                continue
            pY = float(int(fixed[:, Y].sum())) * scale
            pxy = float(int(fixed[X, Y])) * scale + 0.5
            mi += (pxy / den) * math.log(pxy / (pX * pY + 0.25 * ra * rb + 0.5 * ra * pX + 0.5 * rb * pY) * den)
    return mi


def links_stratified(states: np.ndarray, hdw: np.ndarray, pair_a, pair_b, labels, C: int):
    """dict of mi (K, C), mi_all (K,), poly uint8 (K, C), neff (C,), counts and fixed int64 (K, C, 5, 5), frac_bits: what ldw_links_stratified returns."""
    states = np.asarray(states)
    hdw = np.asarray(hdw, dtype=np.float64)
    labels = np.asarray(labels, dtype=np.int64)
    a, b = np.asarray(pair_a, dtype=np.int64), np.asarray(pair_b, dtype=np.int64)
    K = len(a)
    V, F = quantise(hdw)
    sa, sb = np.minimum(states[a], 4).astype(np.int64), np.minimum(states[b], 4).astype(np.int64)
    counts, fixed = np.zeros((K, C, 25), dtype=np.int64), np.zeros((K, C, 25), dtype=np.int64)
    neff = np.zeros(C)
    members = [np.nonzero(labels == c)[0] for c in range(C)]
    for c, mem in enumerate(members):
        neff[c] = float(np.sum(hdw[mem].astype(np.longdouble)))
        if len(mem) == 0:
            continue
        code = sa[:, mem] * 5 + sb[:, mem]
        for k in range(K):
            counts[k, c] = np.bincount(code[k], minlength=25)
            fixed[k, c] = np.rint(np.bincount(code[k], weights=V[mem].astype(np.float64), minlength=25)).astype(np.int64)   # (every sum < 2^52: exact)
    mi, poly = np.zeros((K, C)), np.zeros((K, C), dtype=np.uint8)
    for k in range(K):
        for c in range(C):
            if len(members[c]) == 0:
                continue
            t = counts[k, c].reshape(5, 5)
            poly[k, c] = int((t.sum(axis=1) > 0).sum() > 1) | (int((t.sum(axis=0) > 0).sum() > 1) << 1)
            mi[k, c] = mi_from_tables(counts[k, c], fixed[k, c], F, neff[c])
    neff_all = float(np.sum(hdw[labels >= 0].astype(np.longdouble)))
    mi_all = np.asarray([mi_from_tables(counts[k].sum(axis=0), fixed[k].sum(axis=0), F, neff_all) for k in range(K)])
    return dict(mi=mi, mi_all=mi_all, poly=poly, neff=neff, counts=counts.reshape(K, C, 5, 5), fixed=fixed.reshape(K, C, 5, 5), frac_bits=F)


def summary_columns(mi: np.ndarray, mi_all: np.ndarray, poly: np.ndarray, neff: np.ndarray):
    """The columns link_lineage_mi appends, from the (K, C) matrix: dict of mi_within, within_frac, n_poly, top_cluster, top_share."""
    mi, neff = np.asarray(mi, dtype=np.float64), np.asarray(neff, dtype=np.float64)
    K = mi.shape[0]
    out = dict(mi_within=np.zeros(K), within_frac=np.full(K, np.nan), n_poly=np.zeros(K, dtype=np.int64), top_cluster=np.full(K, -1, dtype=np.int64),
               top_share=np.full(K, np.nan))
    for k in range(K):
        w = neff * mi[k]
        tot = float(w.sum())
        out["mi_within"][k] = tot / float(neff.sum())
        if mi_all[k] > 0:
            out["within_frac"][k] = out["mi_within"][k] / mi_all[k]
        out["n_poly"][k] = int((np.asarray(poly[k]) == 3).sum())
        if tot != 0:
            out["top_cluster"][k] = int(np.argmax(w))
            out["top_share"][k] = float(w.max()) / tot
    return out
