"""Neighbour joining as DESIGN.md 26 states it, in numpy: the reference of tests/test_nj_host.py and tests/test_nj_gpu.py.  Every operation is
one IEEE fp64 operation in the order of the statement (numpy never fuses a product with a sum), so the device result must be bit-identical.
O(n^2) vectorised per join: fine up to a few hundred nodes.  Also here: the matrices the tests use and the patristic distances of a result."""
import numpy as np


def initial_row_sums(d: np.ndarray) -> np.ndarray:
    """r_i = d(0, i) + d(1, i) + ... + d(N-1, i), added in that order."""
    r = np.zeros(d.shape[0], dtype=np.float64)
    for k in range(d.shape[0]):
        r = r + d[k]
    return r


def nj(dist):
    """(parent int32 [2N-2], length float64 [2N-2]) of the N x N matrix: nodes 0 .. N-1 the tips, N + s the node of join s, 2N-3 the root."""
    d = np.array(dist, dtype=np.float64)
    N = d.shape[0]
    assert d.shape == (N, N) and N >= 3
    r = initial_row_sums(d)
    ids = np.arange(N, dtype=np.int64)          # node of every slot (the device compacts its slots another way: the rule is on nodes)
    parent = np.full(2 * N - 2, -1, dtype=np.int32)
    length = np.zeros(2 * N - 2, dtype=np.float64)
    for s in range(N - 3):
        n = N - s
        dd = d[:n, :n]
        q = (float(n - 2) * dd - r[:n, None]) - r[None, :n]
        np.fill_diagonal(q, np.inf)
        qmin = q.min()
        ii, jj = np.nonzero(q == qmin)          # IEEE equality: what ties means
        lo, hi = np.minimum(ids[ii], ids[jj]), np.maximum(ids[ii], ids[jj])
        k = np.lexsort((hi, lo))[0]
        si, sj = int(ii[k]), int(jj[k])
        sa, sb = (si, sj) if ids[si] < ids[sj] else (sj, si)
        a, b, u = int(ids[sa]), int(ids[sb]), N + s
        dab, ra, rb = float(d[sa, sb]), float(r[sa]), float(r[sb])
        la = 0.5 * dab + (ra - rb) / (2.0 * float(n - 2))
        lb = dab - la
        parent[a] = parent[b] = u
        length[a], length[b] = la, lb
        dak, dbk = d[sa, :n].copy(), d[sb, :n].copy()
        duk = ((dak + dbk) - dab) * 0.5
        r[:n] = ((r[:n] - dak) - dbk) + duk
        ru = ((ra + rb) - float(n) * dab) * 0.5
        # u into the lower of the two slots, the last slot into the other one
        su, sd = min(sa, sb), max(sa, sb)
        d[su, :n] = duk
        d[:n, su] = duk
        d[su, su] = 0.0
        r[su] = ru
        ids[su] = u
        last = n - 1
        if sd != last:
            d[sd, :n] = d[last, :n]
            d[:n, sd] = d[:n, last]
            d[sd, sd] = 0.0
            r[sd] = r[last]
            ids[sd] = ids[last]
    o = np.argsort(ids[:3])
    i, j, k = (int(x) for x in o)
    dij, dik, djk = float(d[i, j]), float(d[i, k]), float(d[j, k])
    length[ids[i]] = ((dij + dik) - djk) * 0.5
    length[ids[j]] = ((djk + dij) - dik) * 0.5
    length[ids[k]] = ((dik + djk) - dij) * 0.5
    parent[ids[:3]] = 2 * N - 3
    return parent, length


def patristic(parent, length, tips):
    """Path lengths from each of ``tips`` to every tip 0 .. N-1: float64 [len(tips), N].  A parent has a larger id than its children, so from the
    ancestors of a tip the distances fill downwards by descending id.  Sums are exact when the lengths are dyadic and small."""
    par, ln = np.asarray(parent).tolist(), np.asarray(length).tolist()
    m = len(par)
    N = (m + 2) // 2
    out = np.zeros((len(tips), N))
    for row, t in enumerate(tips):
        dist = [None] * m
        v, acc = int(t), 0.0
        while v >= 0:
            dist[v] = acc
            acc, v = acc + ln[v], par[v]
        for v in range(m - 2, -1, -1):
            if dist[v] is None:
                dist[v] = dist[par[v]] + ln[v]
        out[row] = dist[:N]
    return out


# ---- the matrices of the tests ----------------------------------------------------------------------------------------------------------------------

def random_tree_matrix(N: int, seed: int, denom: int = 8, max_len: int = 16):
    """An additive matrix: the path lengths between the N tips of a random unrooted binary tree whose branches are multiples of 1 / denom
    (at least one unit: the tree is then the only one that fits the matrix).  Exact in fp64."""
    rng = np.random.default_rng(seed)
    # grow the tree by splitting a random branch: edges as (node, node, length)
    edges = [(0, N, 0), (1, N, 0), (2, N, 0)] if N >= 3 else []
    nxt = N + 1
    for t in range(3, N):
        e = int(rng.integers(len(edges)))
        x, y, _ = edges[e]
        edges[e] = (x, nxt, 0)
        edges.append((nxt, y, 0))
        edges.append((t, nxt, 0))
        nxt += 1
    # all node-to-node path lengths, one node at a time outwards from node N: a new node is its neighbour's row plus the branch between them
    adj = [[] for _ in range(nxt)]
    for x, y, _ in edges:
        w = int(rng.integers(1, max_len + 1)) / denom
        adj[x].append((y, w))
        adj[y].append((x, w))
    full = np.zeros((nxt, nxt))
    seen, stack = [N], [N]
    while stack:
        v = stack.pop()
        for u, w in adj[v]:
            if u != N and not full[u, N]:
                full[u, seen] = full[v, seen] + w
                full[seen, u] = full[u, seen]
                seen.append(u)
                stack.append(u)
    return np.ascontiguousarray(full[:N, :N])


def tie_matrix(N: int, seed: int):
    """Symmetric, integer entries 0 .. 3, zero diagonal: exact ties by the hundred and negative branches."""
    rng = np.random.default_rng(seed)
    m = np.triu(rng.integers(0, 4, (N, N)), 1).astype(np.float64)
    return m + m.T


def last_first_matrix(N: int):
    """The largest ids join first: a caterpillar, tip i on spine node i by a unit branch, the spine edge from i to i + 1 of length i + 1.  The pair
    (N-2, N-1) joins first, then N-3 with the new node, and so on down: in every one of these joins b sits in the last slot."""
    x = np.concatenate([[0.0], np.cumsum(np.arange(1.0, N))])
    d = np.abs(x[:, None] - x[None, :]) + 2.0
    np.fill_diagonal(d, 0.0)
    return d


def last_slot_a_matrix(N: int):
    """``last_first_matrix`` with its tips renamed so that tips 0 and 1 join first (the last slot's tip N-1 moves into tip 1's slot) and tip N-2, now
    in the last slot, joins the new node next: a, the smaller id, sits in the last slot.  N >= 6."""
    pos = np.arange(N) - 2
    pos[0], pos[1], pos[N - 2], pos[N - 1] = N - 1, N - 2, N - 3, N - 4
    return last_first_matrix(N)[np.ix_(pos, pos)]
