"""The co-change scan restated in numpy (include/ldweaver_amd.h 23): what ldw_tree_cochange_scan / ldw_tree_cochange_links and their debug
entries are pinned against, integer for integer.  It works from a bool change matrix (``parsimony(...)["change"]`` of tests/pars_ref.py) or from bitmaps.

The M slots are the eligible SNPs in ascending order: ``changes[M]``, ``idx[M]`` (their global SNP), ``pos[M]``.  co = C @ C.T on int64; a pair a < b of
slots is in P where ``min_len`` < 0 or circ_len(pos[b], pos[a], g) > min_len; it qualifies when co B >= min_lift changes[a] changes[b]."""
import numpy as np

BINS = 1024


def circ_len(pos1, pos2, g):
    """csrc/ldw_dev.h, operation by operation: len = 0.5 g - |(pos1 - pos2) mod g - 0.5 g| with R's floored mod."""
    x = np.asarray(pos1, dtype=np.float64) - np.asarray(pos2, dtype=np.float64)
    g = float(g)
    d = x - np.floor(x / g) * g
    d = np.where(d < 0, d + g, d)
    d = np.where(d >= g, d - g, d)
    return 0.5 * g - np.abs(d - 0.5 * g)


def unpack_bits(bits):
    """bool (M, 32 words) from uint32 bitmaps (words, M): bit v of a row is bit v & 31 of word v >> 5."""
    w = np.asarray(bits, dtype=np.uint32)
    words, M = w.shape
    out = ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool)       # (words, M, 32)
    return np.ascontiguousarray(out.transpose(1, 0, 2).reshape(M, words * 32))


def pack_bits(change):
    """uint32 bitmaps (words, M) of a bool matrix (M, nodes): the layout k_pars_down leaves."""
    c = np.asarray(change, dtype=bool)
    M, nodes = c.shape
    words = (nodes + 31) // 32
    pad = np.zeros((M, words * 32), dtype=np.uint64)
    pad[:, :nodes] = c
    w = (pad.reshape(M, words, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    return np.ascontiguousarray(w.T)


def co_matrix(change):
    c = np.asarray(change, dtype=bool).astype(np.int64)
    return c @ c.T


def pair_sets(co, changes, B, min_lift=0, min_len=-1.0, pos=None, g=None):
    """(in_p, qualifies): bool (M, M) over a < b."""
    M = co.shape[0]
    ch = np.asarray(changes, dtype=np.int64)
    in_p = np.triu(np.ones((M, M), dtype=bool), 1)
    if min_len >= 0:
        p = np.asarray(pos, dtype=np.float64)
        in_p &= circ_len(p[None, :], p[:, None], g) > min_len                      # [a][b]: circ_len(pos[b], pos[a], g)
    q = in_p & (co * int(B) >= int(min_lift) * ch[:, None] * ch[None, :])
    return in_p, q


def scan(change, changes, B, min_co=0, min_lift=0, min_len=-1.0, pos=None, g=None):
    """dict of hist uint64 (1024), best int32 (M), nge int64 (M), npairs, n_qualifying — over the M slots."""
    co = co_matrix(change)
    M = co.shape[0]
    in_p, q = pair_sets(co, changes, B, min_lift, min_len, pos, g)
    hist = np.bincount(np.minimum(co[q], BINS - 1), minlength=BINS).astype(np.uint64)
    both = q | q.T                                                                 # every pair adds to both of its SNPs
    best = np.where(both.any(axis=1), np.where(both, co, -1).max(axis=1, initial=-1), -1).astype(np.int32)
    nge = (both & (co >= int(min_co))).sum(axis=1).astype(np.int64)
    return dict(hist=hist, best=best.reshape(M), nge=nge.reshape(M), npairs=int(in_p.sum()), n_qualifying=int(q.sum()), co=co, q=q)


def links(change, changes, idx, B, min_co=0, min_lift=0, min_len=-1.0, pos=None, g=None, best_in=None):
    """dict of a, b (global SNPs, a < b), co — sorted by (a, b) —, count, and partner int32 (M) (global SNPs, -1: none; None without best_in)."""
    co = co_matrix(change)
    M = co.shape[0]
    ix = np.asarray(idx, dtype=np.int64)
    _, q = pair_sets(co, changes, B, min_lift, min_len, pos, g)
    sa, sb = np.nonzero(q & (co >= int(min_co)))
    partner = None
    if best_in is not None:
        bi = np.asarray(best_in, dtype=np.int64)
        both = q | q.T
        match = both & (co == bi[:, None]) & (bi[:, None] >= 0)
        partner = np.full(M, -1, dtype=np.int32)
        if M:
            first = match.argmax(axis=1)                                           # the slots ascend with the SNPs: the first match is the smallest
            partner = np.where(match.any(axis=1), ix[first], -1).astype(np.int32)
    return dict(a=ix[sa].astype(np.int32), b=ix[sb].astype(np.int32), co=co[sa, sb].astype(np.int32), count=len(sa), partner=partner)


def eligible(score, min_changes):
    return np.flatnonzero(np.asarray(score) >= int(min_changes)).astype(np.int32)


def tree_scan(change, score, B, min_changes=2, min_co=2, min_lift=0, min_len=-1.0, POS=None, g=None):
    """What ldw_tree_cochange_scan gives over all L SNPs, from ``parsimony(...)``'s change (L, nodes) and score."""
    L = len(score)
    idx = eligible(score, min_changes)
    r = scan(change[idx], np.asarray(score)[idx], B, min_co, min_lift, min_len, None if POS is None else np.asarray(POS)[idx], g)
    best, nge = np.full(L, -1, dtype=np.int32), np.zeros(L, dtype=np.int64)
    best[idx], nge[idx] = r["best"], r["nge"]
    return dict(changes=np.asarray(score, dtype=np.int32), hist=r["hist"], best=best, nge=nge, npairs=r["npairs"], n_qualifying=r["n_qualifying"], idx=idx)


def tree_links(change, score, B, min_changes=2, min_co=2, min_lift=0, min_len=-1.0, POS=None, g=None, best_in=None):
    L = len(score)
    idx = eligible(score, min_changes)
    r = links(change[idx], np.asarray(score)[idx], idx, B, min_co, min_lift, min_len, None if POS is None else np.asarray(POS)[idx], g,
              None if best_in is None else np.asarray(best_in)[idx])
    if best_in is not None:
        partner = np.full(L, -1, dtype=np.int32)
        partner[idx] = r["partner"]
        r["partner"] = partner
    return r


def sorted_links(d):
    """(a, b, co) of a links dict in (a, b) order: the device lists come in no stated order."""
    a, b, co = (np.asarray(d[k]) if d[k] is not None else np.zeros(0, dtype=np.int32) for k in ("a", "b", "co"))
    o = np.lexsort((b, a))
    return a[o], b[o], co[o]


def planted_example():
    """The example of the issue that opened the scan: 64 tips on a balanced tree, 40 SNPs, seed 7.  SNPs 0-9 flip on one depth-1 branch (lineage markers),
    SNPs 10 and 11 flip in the same four depth-4 clades (the planted pair), every other SNP flips in two random clades of depth >= 3; 5 % of the cells are N.
    Returns (parent, tip_seq, states uint8 (40, 64))."""
    import pars_ref as R
    rng = np.random.default_rng(7)
    n, Ls = 64, 40
    parent, tip_seq = R.balanced(list(range(n)))
    nodes = len(parent)
    depth = np.zeros(nodes, dtype=np.int64)
    for v in range(1, nodes):
        depth[v] = depth[parent[v]] + 1
    kids = R.children_of(parent)

    def tips_under(v):
        out, stack = [], [v]
        while stack:
            u = stack.pop()
            if kids[u]:
                stack.extend(kids[u])
            else:
                out.append(int(tip_seq[u]))
        return out

    states = np.zeros((Ls, n), dtype=np.uint8)
    d1 = [v for v in range(nodes) if depth[v] == 1]
    d4 = [v for v in range(nodes) if depth[v] == 4]
    deep = [v for v in range(nodes) if depth[v] >= 3 and kids[v]]
    for i in range(10):
        states[i, tips_under(d1[0])] = 1
    # four depth-4 clades no two of which are sisters: four separate changes whatever the reconstruction
    four = [d4[0], d4[2], d4[5], d4[9]]
    for i in (10, 11):
        for v in four:
            states[i, tips_under(v)] = 1
    for i in range(12, Ls):
        for v in rng.choice(len(deep), size=2, replace=False):
            states[i, tips_under(deep[int(v)])] ^= 1
    states[rng.random((Ls, n)) < 0.05] = 4
    return parent, tip_seq, states
