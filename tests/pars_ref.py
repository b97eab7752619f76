"""Maximum parsimony on a given tree, restated in numpy (include/ldweaver_amd.h 17): what the device is pinned against, integer for
integer.  The loops run over the nodes and are vectorised over the SNP columns.  ``sankoff_min`` is the exact per-state dynamic programme for the
least number of changes of one column, which the statement's score and its down pass must both equal (tests/test_parsimony_host.py).

The tree: ``parent[nodes]`` with ``parent[0] = -1`` and ``0 <= parent[v] < v``; ``tip_seq[nodes]`` the sequence of a node without children, -1 at a
node with children.  ``states`` is the alignment, uint8 (L, N), values 0..4 = A, C, G, T, N.  A set is a mask: bit s stands for state s."""
import numpy as np

WILDCARD = 0x0F
BITS = np.arange(5, dtype=np.uint8)


def children_of(parent):
    kids = [[] for _ in parent]
    for v in range(1, len(parent)):
        kids[int(parent[v])].append(v)
    return kids


def tip_sets(states, seq, gap_mode):
    """The sets of one tip for all columns: {A, C, G, T} for N under gap_mode 0, else {s}."""
    s = np.asarray(states)[:, int(seq)].astype(np.uint8)
    one = (np.uint8(1) << s).astype(np.uint8)
    return np.where((s == 4) & (gap_mode == 0), np.uint8(WILDCARD), one).astype(np.uint8)


def up_pass(parent, tip_seq, states, gap_mode=0):
    """Hartigan's rule from the last node to the first: (sets uint8 (nodes, L), score int32 (L))."""
    nodes, L = len(parent), np.asarray(states).shape[0]
    kids = children_of(parent)
    sets = np.zeros((nodes, L), dtype=np.uint8)
    score = np.zeros(L, dtype=np.int32)
    for v in range(nodes - 1, -1, -1):
        if not kids[v]:
            sets[v] = tip_sets(states, tip_seq[v], gap_mode)
            continue
        c = np.zeros((L, 5), dtype=np.int64)
        for u in kids[v]:
            c += (sets[u][:, None] >> BITS) & 1
        K = c.max(axis=1)
        sets[v] = (((c == K[:, None]).astype(np.uint8)) << BITS).sum(axis=1).astype(np.uint8)
        score += (len(kids[v]) - K).astype(np.int32)
    return sets, score


def low_state(sets):
    """The lowest state of every (non-empty) set."""
    s = np.asarray(sets).astype(np.int64)
    return np.round(np.log2(s & -s)).astype(np.uint8)


def down_pass(parent, sets):
    """(state uint8 (nodes, L), change bool (nodes, L)): node 0 takes the lowest state of its set, any other node its parent's state where its set
    holds it, else the lowest of its set; ``change[v]``: branch v carries a change (never at v = 0)."""
    nodes, L = sets.shape
    state = np.zeros((nodes, L), dtype=np.uint8)
    change = np.zeros((nodes, L), dtype=bool)
    state[0] = low_state(sets[0])
    for v in range(1, nodes):
        up = state[int(parent[v])]
        keep = ((sets[v] >> up) & 1).astype(bool)
        state[v] = np.where(keep, up, low_state(sets[v]))
        change[v] = state[v] != up
    return state, change


def min_changes(tip_seq, states, gap_mode=0):
    """Distinct states at the tree's tips minus one, floored at 0; N is not counted under gap_mode 0."""
    seqs = [int(s) for s in tip_seq if s >= 0]
    sub = np.asarray(states)[:, seqs]
    n = np.zeros(sub.shape[0], dtype=np.int32)
    for s in range(5 if gap_mode == 1 else 4):
        n += (sub == s).any(axis=1)
    return np.maximum(n - 1, 0).astype(np.int32)


def parsimony(parent, tip_seq, states, gap_mode=0):
    """Everything the three entry points give, for all columns: dict of score, min_changes (int32 (L)), state (uint8 (L, nodes)), change (bool
    (L, nodes))."""
    sets, score = up_pass(parent, tip_seq, states, gap_mode)
    state, change = down_pass(parent, sets)
    return dict(score=score, min_changes=min_changes(tip_seq, states, gap_mode), state=np.ascontiguousarray(state.T), change=np.ascontiguousarray(change.T))


def cochanges(change, a, b):
    """(changes_a, changes_b, co) int32 of the pairs (a[i], b[i]) from ``parsimony(...)["change"]``."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    n = change.sum(axis=1).astype(np.int32)
    co = np.array([int(np.count_nonzero(change[x] & change[y])) for x, y in zip(a.tolist(), b.tolist())], dtype=np.int32).reshape(len(a))
    return n[a], n[b], co


def sankoff_min(parent, tip_seq, column, gap_mode=0):
    """The least number of changes of one column (states by sequence) over ALL assignments of the five states to the nodes with children: cost[v][s] =
    the sum over the children u of min_t(cost[u][t] + [t != s]); a tip costs 0 in the states of its set and is impossible elsewhere."""
    INF = 1 << 40
    nodes = len(parent)
    kids = children_of(parent)
    cost = [[0] * 5 for _ in range(nodes)]
    for v in range(nodes - 1, -1, -1):
        if not kids[v]:
            s = int(column[int(tip_seq[v])])
            m = WILDCARD if (s == 4 and gap_mode == 0) else 1 << s
            cost[v] = [0 if (m >> x) & 1 else INF for x in range(5)]
            continue
        for s in range(5):
            cost[v][s] = sum(min(cost[u][t] + (t != s) for t in range(5)) for u in kids[v])
    return min(cost[0])


# ---- trees for the tests: each returns (parent int32 [nodes], tip_seq int32 [nodes]) over the sequences `seqs` (a list, in tip order) --------------------

def finish(parent, seqs):
    parent = np.asarray(parent, dtype=np.int32)
    has_kid = np.zeros(len(parent), dtype=bool)
    has_kid[parent[1:]] = True
    tip_seq = np.full(len(parent), -1, dtype=np.int32)
    tips = np.flatnonzero(~has_kid)
    assert len(tips) == len(seqs), (len(tips), len(seqs))
    tip_seq[tips] = np.asarray(seqs, dtype=np.int32)
    return parent, tip_seq


def caterpillar(seqs):
    """As deep as a tree of these tips gets: every node with children has a tip and the rest of the tree under it."""
    n, parent = len(seqs), [-1]
    spine = 0
    for k in range(n - 1):
        parent.append(spine)                  # a tip
        parent.append(spine)                  # the next spine node, or the last tip
        if k < n - 2:
            spine = len(parent) - 1
    return finish(parent, seqs)


def balanced(seqs):
    parent = [-1]

    def grow(v, n):
        if n == 1:
            return
        for m in (n // 2, n - n // 2):
            parent.append(v)
            grow(len(parent) - 1, m)

    grow(0, len(seqs))                        # (depth log2 n)
    return finish(parent, seqs)


def star(seqs):
    return finish([-1] + [0] * len(seqs), seqs)


def random_tree(rng, seqs, max_arity=None, p_unary=0.0):
    """A random tree over the tips: groups of 2 .. max_arity loose nodes are hung under a new node until one node is left; with probability p_unary a new
    node gets a single-child node above it.  Renumbered so that a parent comes before its children."""
    n = len(seqs)
    max_arity = n if max_arity is None else max_arity
    kids, loose = {}, list(range(n))
    nxt = n
    while len(loose) > 1:
        k = int(rng.integers(2, min(max_arity, len(loose)) + 1))
        pick = [loose.pop(int(rng.integers(len(loose)))) for _ in range(k)]
        kids[nxt] = pick
        top = nxt
        nxt += 1
        if rng.random() < p_unary:
            kids[nxt] = [top]
            top = nxt
            nxt += 1
        loose.append(top)
    root = loose[0]
    if root < n:                               # (a single tip: cannot happen for n >= 2)
        raise ValueError("a tree needs two tips")
    order, parent, stack = [], [], [(root, -1)]
    tip_of = []
    while stack:
        v, p = stack.pop()
        me = len(order)
        order.append(v)
        parent.append(p)
        if v < n:
            tip_of.append(v)
        for u in reversed(kids.get(v, [])):
            stack.append((u, me))
    return finish(parent, [seqs[t] for t in tip_of])


def from_tree(tree, seqs=None):
    """(parent, tip_seq) of a ``ldweaver_amd.tree.Tree`` whose tip t stands for sequence seqs[t] (default: t)."""
    tip_seq = np.full(tree.n_nodes, -1, dtype=np.int32)
    tip_seq[tree.tip_node] = np.arange(tree.n_tips, dtype=np.int32) if seqs is None else np.asarray(seqs, dtype=np.int32)
    return np.asarray(tree.parent, dtype=np.int32), tip_seq


def random_alignment(rng, L, N, p_n=0.2):
    """Random five-state columns with a share p_n of N; where L allows, column 0 is constant, column 1 all N, column 2 one state plus N."""
    st = rng.integers(0, 4, size=(L, N)).astype(np.uint8)
    st[rng.random((L, N)) < p_n] = 4
    if L > 3:
        st[0] = 2
        st[1] = 4
        st[2] = np.where(rng.random(N) < 0.5, 1, 4)
    return st
