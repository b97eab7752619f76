"""The host side of the neighbour-joining tree, without a GPU: the numpy statement of the algorithm (tests/nj_ref.py) on matrices
whose tree is known, write_newick against parse_newick, the clamp of negative branches, the package's exports."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nj_ref                                                                                   # noqa: E402
from ldweaver_amd.tree import (midpoint_root, nj_clamp, parse_newick, read_newick, tree_from_joins, write_newick)   # noqa: E402


@pytest.mark.parametrize("N", [5, 17, 64, 129])
def test_reference_recovers_additive_trees(N):
    """Branches are multiples of 1/8, so the matrix, every Q and every update are exact: neighbour joining must return THE tree, i.e. the path
    lengths of its result equal the matrix entry for entry."""
    d = nj_ref.random_tree_matrix(N, seed=N)
    parent, length = nj_ref.nj(d)
    assert parent[2 * N - 3] == -1 and np.all(parent[:2 * N - 3] >= N) and np.all(length >= 0)
    assert np.array_equal(nj_ref.patristic(parent, length, range(N)), d)
    tree = tree_from_joins(parent, length, clamp_negative=False)
    assert tree.n_tips == N and tree.n_nodes == 2 * N - 2 and len(tree.children(0)) == 3


def test_reference_id_rule_on_the_zero_matrix():
    parent, length = nj_ref.nj(np.zeros((33, 33)))
    assert parent[:8].tolist() == [33, 33, 34, 34, 35, 35, 36, 36] and not length.any()


def test_special_matrices_join_where_they_say():
    for N in (6, 9, 64):
        p, _ = nj_ref.nj(nj_ref.last_first_matrix(N))
        assert p[N - 1] == p[N - 2] == N and p[N - 3] == p[N] == N + 1
        p, _ = nj_ref.nj(nj_ref.last_slot_a_matrix(N))
        assert p[0] == p[1] == N and p[N - 2] == p[N] == N + 1


def test_newick_round_trip(tmp_path):
    d = nj_ref.random_tree_matrix(17, seed=3)
    parent, length = nj_ref.nj(d)
    length = length.copy()
    length[4] = 1e-05
    length[5] = 0.1 + 0.2            # 0.30000000000000004: needs all 17 digits
    length[6] = 123456789.125
    labels = [f"iso_{k}" for k in range(17)]
    labels[2], labels[3], labels[7], labels[9] = "it's (odd), this: one", "with space", "semi;colon", "[bracket]"
    tree = midpoint_root(tree_from_joins(parent, length, labels))
    text = write_newick(tree, tmp_path / "t.nwk")
    assert "1e-05" in text and "'it''s (odd), this: one'" in text and text.endswith(";\n")
    for back in (parse_newick(text.encode()), read_newick(tmp_path / "t.nwk")):
        assert np.array_equal(back.parent, tree.parent)
        assert back.length.tobytes() == tree.length.tobytes()
        assert back.tip_label == [tree.tip_label[t] for t in tree.tip_order()]      # (a file's tips are numbered in its own order)
        assert np.array_equal(back.tip_node, np.sort(tree.tip_node))
        assert np.array_equal(back.child_ptr, tree.child_ptr) and np.array_equal(back.child_idx, tree.child_idx)
    with pytest.raises(ValueError):
        write_newick(tree_from_joins(parent, length, [""] + labels[1:]))


def test_clamp_on_a_hand_made_join():
    """Four tips; join 0 makes node 4 of tips 0 and 1 with la = -0.5, lb = 2.5 (d_ab = 2); at the root tip 2 has -0.25."""
    parent = np.array([4, 4, 5, 5, 5, -1], dtype=np.int32)
    length = np.array([-0.5, 2.5, -0.25, 1.0, 0.75, 0.0])
    out = nj_clamp(parent, length)
    assert out.tolist() == [0.0, 2.0, 0.0, 1.0, 0.75, 0.0] and length[0] == -0.5
    length = np.array([2.5, -0.5, 0.5, 1.0, 0.75, 0.0])
    assert nj_clamp(parent, length).tolist() == [2.0, 0.0, 0.5, 1.0, 0.75, 0.0]
    assert tree_from_joins(parent, length).length.min() == 0.0
    assert tree_from_joins(parent, length, clamp_negative=False).length.min() == -0.5


def test_clamp_on_a_tie_heavy_matrix():
    parent, length = nj_ref.nj(nj_ref.tie_matrix(65, seed=1))
    neg = int((length < 0).sum())
    assert neg >= 24, neg      # dozens
    with pytest.raises(ValueError):
        midpoint_root(tree_from_joins(parent, length, clamp_negative=False))
    out = nj_clamp(parent, length)
    assert out.min() >= 0
    for u in range(65, 2 * 65 - 3):     # the two branches under a join still add up to d_ab
        a, b = np.nonzero(parent == u)[0]
        assert out[a] + out[b] == length[a] + length[b]
    rooted = midpoint_root(tree_from_joins(parent, length))
    assert rooted.n_tips == 65


def test_package_exports():
    import ldweaver_amd
    from ldweaver_amd import tree
    assert ldweaver_amd.nj_tree is tree.nj_tree and ldweaver_amd.write_newick is tree.write_newick
    assert {"nj_tree", "write_newick"} <= set(ldweaver_amd.__all__)
