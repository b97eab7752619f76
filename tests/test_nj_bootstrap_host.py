"""Bootstrap support of the neighbour-joining tree, the parts that need no GPU: the diagonal identity the device's distances rest on,
the numpy reference's support on a case made by hand, the multiplicities, support through Newick, rooting, ordering and the layout."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nj_boot_ref as BR                                   # noqa: E402
from ldweaver_amd import tree as T                         # noqa: E402


def test_diagonal_identity_is_the_definition():
    st = BR.five_state_alignment(L=120, N=37, seed=3)
    kinds = {len(np.unique(st[a])) for a in range(st.shape[0])}
    assert 1 in kinds and 2 in kinds and max(kinds) >= 3
    rng = np.random.default_rng(4)
    for m in (np.ones(120, dtype=np.int64), rng.integers(0, 64, size=120), np.full(120, 63), (np.arange(120) == 5) * 63):
        want = BR.weighted_distance(st, m)
        got = BR.identity_distance(st, m)
        assert np.array_equal(got, want)
        assert np.array_equal(want, want.T) and not np.diag(want).any()
    assert np.array_equal(BR.weighted_distance(st, np.ones(120)), (st[:, :, None] != st[:, None, :]).sum(axis=0))


def test_support_by_hand():
    # N = 5: nodes 5, 6 are the joins, 7 the root.  The reference joins (0, 1) then (2, 3); tip 4, node 5 and node 6 hang on the root
    ref = np.array([5, 5, 6, 6, 7, 7, 7, -1], dtype=np.int32)
    assert BR.splits(ref) == {frozenset([2, 3, 4]): 5, frozenset([2, 3]): 6}
    same_splits = np.array([6, 6, 5, 5, 7, 7, 7, -1], dtype=np.int32)      # (2, 3) first, then (0, 1): the same two splits from other nodes
    other = np.array([5, 6, 5, 6, 7, 7, 7, -1], dtype=np.int32)            # (0, 2) and (1, 3): neither split
    half = np.array([5, 5, 7, 6, 6, 7, 7, -1], dtype=np.int32)             # (0, 1) and (3, 4): the first split alone
    assert BR.support(ref, [same_splits, other]).tolist() == [-1, -1, -1, -1, -1, 1, 1, -1]
    assert BR.support(ref, [same_splits, other, half, ref]).tolist() == [-1, -1, -1, -1, -1, 3, 2, -1]
    assert BR.support(np.array([3, 3, 3, -1]), [np.array([3, 3, 3, -1])]).tolist() == [-1, -1, -1, -1]


def test_bootstrap_multiplicities():
    m = T.bootstrap_multiplicities(50, 7, seed=1)
    assert m.shape == (7, 50) and m.dtype == np.int32 and m.min() >= 0
    assert m.sum(axis=1).tolist() == [50] * 7
    assert np.array_equal(m, T.bootstrap_multiplicities(50, 7, seed=1))
    assert not np.array_equal(m, T.bootstrap_multiplicities(50, 7, seed=2))
    rng = np.random.default_rng(1)
    assert np.array_equal(m[0], np.bincount(rng.integers(0, 50, size=50), minlength=50))
    assert np.array_equal(m[1], np.bincount(rng.integers(0, 50, size=50), minlength=50))
    assert len({r.tobytes() for r in m}) == 7


def _split_support(tree: T.Tree) -> dict:
    """{split, as the frozenset of tip labels on the side without the first label in sorted order: support} over the branches that have one."""
    n = tree.n_nodes
    label_of = {int(v): tree.tip_label[t] for t, v in enumerate(tree.tip_node.tolist())}
    below = [frozenset([label_of[v]]) if v in label_of else frozenset() for v in range(n)]
    par = tree.parent.tolist()
    for v in range(n - 1, 0, -1):
        below[par[v]] = below[par[v]] | below[v]
    everything, first = below[0], min(tree.tip_label)
    out = {}
    for v in range(1, n):
        if tree.support is not None and tree.support[v] >= 0:
            s = everything - below[v] if first in below[v] else below[v]
            assert out.setdefault(s, int(tree.support[v])) == int(tree.support[v]), "two branches of one split disagree"
    return out


def _random_supported_tree(seed: int, n: int):
    """A random NJ-shaped tree (joins of random pairs) with random support on its n - 3 internal branches and positive lengths."""
    rng = np.random.default_rng(seed)
    active = list(range(n))
    parent = np.full(2 * n - 2, -1, dtype=np.int32)
    for s in range(n - 3):
        i, j = sorted(rng.choice(len(active), 2, replace=False).tolist())
        parent[active[i]] = parent[active[j]] = n + s
        active = [v for k, v in enumerate(active) if k not in (i, j)] + [n + s]
    parent[active] = 2 * n - 3
    length = rng.integers(1, 9, size=2 * n - 2) / 4.0
    length[2 * n - 3] = 0.0
    support = np.full(2 * n - 2, -1, dtype=np.int32)
    support[n:2 * n - 3] = rng.integers(0, 101, size=n - 3)
    return T.tree_from_joins(parent, length, [f"t{k:02d}" for k in range(n)], True, support, 100)


def test_tree_support_defaults_to_none():
    t = T.parse_newick(b"((a:1,b:1):1,c:2,d:1);")
    assert t.support is None and t.n_replicates is None
    assert T.midpoint_root(t).support is None and T.ladderize(t).support is None
    assert T.tree_from_joins([4, 4, 5, 5, 5, -1], [1.0, 1, 1, 1, 1, 0]).support is None


def test_newick_round_trip_keeps_support():
    t = _random_supported_tree(1, 12)
    assert t.n_replicates == 100 and (t.support[t.tip_node] == -1).all() and t.support[0] == -1
    assert sorted(t.support[t.support >= 0].tolist()) == sorted(_split_support(t).values()) and len(_split_support(t)) == 9
    text = T.write_newick(t)
    back = T.parse_newick(text.encode())
    assert np.array_equal(back.parent, t.parent) and np.array_equal(back.length, t.length)
    assert [back.tip_label[k] for k in back.tip_order()] == [t.tip_label[k] for k in t.tip_order()]      # (a file numbers its tips in its own order)
    assert back.support.dtype == np.int32 and np.array_equal(back.support, t.support) and _split_support(back) == _split_support(t)
    assert T.write_newick(back) == text
    assert T.parse_newick(b"((a:1,b:1)87:0.25,c:2,d:1);").support.tolist() == [-1, 87, -1, -1, -1, -1]
    assert ")87:0.25" in T.write_newick(T.parse_newick(b"((a:1,b:1)87:0.25,c:2,d:1);"))


def test_newick_without_integer_labels_has_no_support():
    for text in (b"((a:1,b:1):0.25,c:2,d:1);", b"((a:1,b:1)clade:0.25,c:2,d:1);", b"((a:1,b:1)0.87:0.25,c:2,d:1);", b"((a:1,b:1)'87':0.25,c:2,d:1);",
                 b"((a:1,b:1)-3:0.25,c:2,d:1);", b"((a:1,b:1):0.25,c:2,d:1)99;"):
        t = T.parse_newick(text)
        assert t.support is None, text
        assert t.parent.tolist() == [-1, 0, 1, 1, 0, 0] and t.length.tolist() == [0.0, 0.25, 1.0, 1.0, 2.0, 1.0]
    mixed = T.parse_newick(b"(((a:1,b:1)x:1,e:1)5:1,c:2,d:1);")
    assert mixed.support.tolist() == [-1, 5, -1, -1, -1, -1, -1, -1]


@pytest.mark.parametrize("seed", [2, 3, 4, 5])
def test_rooting_and_ladderizing_carry_support(seed):
    t = _random_supported_tree(seed, 14)
    want = _split_support(t)
    assert len(want) == 11
    rooted = T.midpoint_root(t)
    assert _split_support(rooted) == want and rooted.n_replicates == 100
    lad = T.ladderize(rooted)
    assert _split_support(lad) == want and lad.n_replicates == 100
    assert (lad.support[lad.tip_node] == -1).all() and lad.support[0] == -1


def test_midpoint_inside_a_branch_and_an_old_root_removed():
    # the midpoint of a - d (path 1 + 3 + 4 + 1 = 9) lies inside the branch of length 4, whose support is 60: both halves keep it
    t = T.parse_newick(b"((a:1,b:1)80:3,c:1,(d:1,e:1)60:4);")
    r = T.midpoint_root(t)
    assert r.n_nodes == t.n_nodes + 1 and len(r.children(0)) == 2
    assert _split_support(r) == _split_support(t) == {frozenset("de"): 60, frozenset("cde"): 80}
    halves = [v for v in r.children(0).tolist()]
    assert sorted(r.support[halves].tolist()) == [60, 60] and sorted(r.length[halves].tolist()) == [0.5, 3.5]
    # a rooted binary file: the old root's two branches are one split and become one branch, with the larger of the two counts
    t = T.parse_newick(b"((a:1,b:1)70:1,((c:1,d:1)90:1,e:9)40:1);")
    r = T.midpoint_root(t)
    assert r.n_nodes == t.n_nodes and _split_support(r) == {frozenset("cde"): 70, frozenset("cd"): 90}
    t = T.parse_newick(b"((a:1,b:1):1,((c:1,d:1)90:1,e:9)40:1);")
    assert _split_support(T.midpoint_root(t)) == {frozenset("cde"): 40, frozenset("cd"): 90}


def test_layout_appends_one_knob_per_marked_node():
    t = T.ladderize(T.midpoint_root(_random_supported_tree(7, 16)))
    plain = T.tree_layout(t, 300, 300)
    assert len(plain["support_nodes"]) == 0
    lay = T.tree_layout(t, 300, 300, support_min=0.5, n_replicates=100)
    internal = np.diff(t.child_ptr) > 0
    marked = np.nonzero(internal & (t.support >= 50))[0]
    assert 0 < len(marked) < internal.sum() and np.array_equal(lay["support_nodes"], marked)
    nb = len(plain["bars"])
    assert len(lay["bars"]) == nb + len(marked) and np.array_equal(lay["bars"][:nb], plain["bars"])
    for bar, v in zip(lay["bars"][nb:].tolist(), marked.tolist()):
        x0, y0, x1, y1 = bar
        assert (x1 - x0, y1 - y0) == (48, 48) and (x0 + 24, y0 + 24) == (lay["node_x"][v], lay["node_y"][v])
    assert len(T.tree_layout(t, 300, 300, support_min=0.0, n_replicates=100)["support_nodes"]) == (internal & (t.support >= 0)).sum()
    assert len(T.tree_layout(t, 300, 300, support_min=1.01, n_replicates=100)["support_nodes"]) == 0
    bare = T.ladderize(T.midpoint_root(T.parse_newick(b"((a:1,b:1):1,c:2,d:1);")))
    assert len(T.tree_layout(bare, 300, 300, support_min=0.5, n_replicates=100)["support_nodes"]) == 0


def test_a_matrix_has_no_columns_to_resample():
    d = np.zeros((4, 4))
    with pytest.raises(ValueError, match="resample"):
        T.nj_tree(dist=d, bootstrap=3)
    with pytest.raises(ValueError, match="resample"):
        T.nj_tree(dist=d, multiplicities=np.ones((2, 5), dtype=np.int32))
    with pytest.raises(ValueError):
        T.nj_tree(bootstrap=3)
