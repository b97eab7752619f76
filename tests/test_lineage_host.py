"""Host: the lineage check — the numpy restatement tests/lineage_ref.py against a breadth-first search and the oracle, the host-side
policy of ldweaver_amd/lineage.py, and what the two entry points refuse without a device."""
import ctypes as C

import numpy as np
import pytest

import ldw_oracle as orc
import lineage_ref as R
from ldweaver_amd import _lib as L
from ldweaver_amd import lineage as G

MI_TIGHT = 1e-10


def random_graph(rng, N, p):
    a = rng.random((N, N)) < p
    a |= a.T
    np.fill_diagonal(a, True)
    return a


def test_union_find_hook_and_jump_and_breadth_first_search_agree_on_random_graphs():
    """300 random graphs of 1 to 80 vertices, from no edge to dense: the three give the same canonical labels."""
    rng = np.random.default_rng(29)
    counts = set()
    for trial in range(300):
        N = int(rng.integers(1, 81))
        a = random_graph(rng, N, float(rng.random()) ** 2 * 4.0 / N)
        u, nu = R.components_union_find(a)
        b, nb = R.components_bfs(a)
        h, nh, _ = R.components_hook_jump(a)
        assert nu == nb == nh and np.array_equal(u, b) and np.array_equal(u, h), trial
        first = [int(np.nonzero(u == c)[0][0]) for c in range(nu)]
        assert first == sorted(first) and first[0] == 0, trial          # numbered in the order of the smallest member
        counts.add(nu)
    assert 1 in counts and len(counts) > 20


@pytest.mark.parametrize("N", (1024, 4096))
def test_hook_and_jump_takes_few_rounds_on_a_path(N):
    """Single linkage makes chains; minimum-label propagation would take N - 1 rounds on one."""
    rng = np.random.default_rng(N)
    for order in (np.arange(N), np.arange(N)[::-1], rng.permutation(N)):
        a = np.zeros((N, N), dtype=bool)
        a[order[:-1], order[1:]] = True
        a |= a.T
        lab, n, rounds = R.components_hook_jump(a)
        assert n == 1 and not lab.any() and rounds <= 13, rounds


def planted(rng, n_per=100, noise=0.05):
    """Two lineages of n_per; SNPs 0, 1: lineage markers; 2, 3: markers with four flips each; 4, 5: noisy copies of one another, independent of lineage."""
    N = 2 * n_per
    lin = np.repeat([0, 1], n_per)
    st = np.zeros((6, N), dtype=np.uint8)
    st[0], st[1] = lin, lin * 2
    st[2], st[3] = lin, lin
    st[2, rng.choice(N, 4, replace=False)] ^= 1
    st[3, rng.choice(N, 4, replace=False)] ^= 1
    st[4] = rng.integers(0, 2, N)
    st[5] = st[4] ^ (rng.random(N) < noise)
    return st, lin


def test_planted_lineage_markers_and_an_epistatic_pair():
    st, lin = planted(np.random.default_rng(7))
    hdw = np.ones(st.shape[1])
    res = R.links_stratified(st, hdw, [0, 2, 4], [1, 3, 5], lin, 2)
    s = R.summary_columns(res["mi"], res["mi_all"], res["poly"], res["neff"])
    assert res["frac_bits"] == 0 and np.array_equal(res["fixed"], res["counts"])
    assert res["mi_all"][0] > 0.6 and abs(s["mi_within"][0]) <= 1e-12 and not res["poly"][0].any() and s["n_poly"][0] == 0
    assert res["mi_all"][1] > 0.3 and s["within_frac"][1] < 0.1
    assert s["within_frac"][2] > 0.9 and s["n_poly"][2] == 2
    # the oracle on the column subsets says the same
    for k, (a, b) in enumerate(((0, 1), (2, 3), (4, 5))):
        for c in range(2):
            sub = st[:, lin == c]
            uqe, r = orc.uqe_r(sub)
            assert abs(res["mi"][k, c] - orc.mi_pair_direct(sub, np.ones(sub.shape[1]), r, uqe, a, b)) < MI_TIGHT, (k, c)
        uqe, r = orc.uqe_r(st)
        assert abs(res["mi_all"][k] - orc.mi_pair_direct(st, hdw, r, uqe, a, b)) < MI_TIGHT, k


def test_reference_mi_per_cluster_is_the_oracle_on_the_subset():
    """Weighted, five states, clusters of every size down to one, -1 labels and an empty cluster id."""
    rng = np.random.default_rng(11)
    Ls, N, Cn = 12, 90, 5
    st = rng.choice(5, size=(Ls, N), p=[0.4, 0.3, 0.15, 0.1, 0.05]).astype(np.uint8)
    st[3] = 2                                                   # monomorphic everywhere
    hdw = 1.0 / rng.integers(1, 9, N)
    lab = rng.choice([-1, 0, 1, 3, 4], size=N, p=[0.1, 0.5, 0.3, 0.09, 0.01]).astype(np.int32)     # (cluster 2 has no member)
    lab[:2] = (4, 3)
    a, b = rng.integers(0, Ls, 20), rng.integers(0, Ls, 20)
    a[0], b[0], a[1], b[1] = 3, 3, 3, 5
    res = R.links_stratified(st, hdw, a, b, lab, Cn)
    V, F = R.quantise(hdw)
    assert res["frac_bits"] == F > 0 and not res["mi"][:, 2].any() and not res["counts"][:, 2].any() and res["neff"][2] == 0
    assert res["mi"][0].tolist() == [0.0] * Cn and np.isfinite(res["mi"]).all()
    for c in (0, 1, 3, 4):
        mem = lab == c
        uqe, r = orc.uqe_r(st[:, mem])
        assert res["neff"][c] == float(np.sum(hdw[mem].astype(np.longdouble)))
        for k in range(20):
            want = orc.mi_pair_direct(st[:, mem], hdw[mem], r, uqe, int(a[k]), int(b[k]))
            assert abs(res["mi"][k, c] - want) < MI_TIGHT, (k, c)
            assert np.array_equal(res["counts"][k, c], orc.joint_counts(st[:, mem], int(a[k]), int(b[k])))
            assert res["poly"][k, c] == int(r[a[k]] > 1) | (int(r[b[k]] > 1) << 1)
    uqe, r = orc.uqe_r(st[:, lab >= 0])
    for k in range(20):
        assert abs(res["mi_all"][k] - orc.mi_pair_direct(st[:, lab >= 0], hdw[lab >= 0], r, uqe, int(a[k]), int(b[k]))) < MI_TIGHT


def test_min_size_drops_or_pools_and_renumbers():
    lab = np.array([0, 1, 1, 2, 3, 3, 3, 4, 1, -1], dtype=np.int32)           # sizes 1, 3, 1, 3, 1
    out, sizes = G.apply_min_size(lab, 1, "drop")
    assert np.array_equal(out, lab) and sizes.tolist() == [1, 3, 1, 3, 1]
    out, sizes = G.apply_min_size(lab, 2, "drop")
    assert out.tolist() == [-1, 0, 0, -1, 1, 1, 1, -1, 0, -1] and sizes.tolist() == [3, 3]
    out, sizes = G.apply_min_size(lab, 2, "pool")
    assert out.tolist() == [2, 0, 0, 2, 1, 1, 1, 2, 0, -1] and sizes.tolist() == [3, 3, 3]
    out, sizes = G.apply_min_size(lab, 4, "pool")                               # nothing is large enough: one pool
    assert out.tolist() == [0] * 9 + [-1] and sizes.tolist() == [9]
    out, sizes = G.apply_min_size(lab, 4, "drop")
    assert out.tolist() == [-1] * 10 and sizes.tolist() == []
    out, sizes = G.apply_min_size(lab, 3, "pool")
    assert out.dtype == np.int32 and sizes.dtype == np.int64
    with pytest.raises(ValueError):
        G.apply_min_size(lab, 2, "merge")


def test_labels_by_name_in_order_of_first_appearance_with_missing_values():
    import pandas as pd
    names = ["s4", "s2", "s9", "s3", "s1"]
    ser = pd.Series(["x", "y", None, "x"], index=["s1", "s2", "s3", "s4"])
    lab, Cn = G.cluster_labels(ser, names)
    assert lab.tolist() == [0, 1, -1, -1, 0] and Cn == 2 and lab.dtype == np.int32
    frame = pd.DataFrame({"ID": ser.index, "cluster": ser.values, "other": 1})
    assert G.cluster_labels(frame, names)[0].tolist() == lab.tolist()
    lab, Cn = G.cluster_labels([5.0, np.nan, 3.0, 5.0])
    assert lab.tolist() == [0, -1, 1, 0] and Cn == 2
    with pytest.raises(ValueError):
        G.cluster_labels([1, 2, 3], names)
    with pytest.raises(ValueError):
        G.cluster_labels(ser)
    sc = G.SeqClusters(np.array([0, 1, 0, -1], dtype=np.int32), np.array([2, 1]), 30, ["a", "b", "c", "d"])
    assert G.cluster_labels(sc)[1] == 2 and sc.n_clusters == 2
    f = sc.frame()
    assert list(f.columns) == ["ID", "cluster"] and f["ID"].tolist() == ["a", "b", "c", "d"] and f["cluster"].tolist() == [0, 1, 0, -1]


def test_summary_columns_on_a_hand_made_matrix():
    mi = np.array([[0.2, 0.0, 0.1], [0.0, 0.0, 0.0], [0.0, 0.5, 0.0], [0.1, 0.1, 0.1]])
    neff = np.array([10.0, 20.0, 0.0])                     # (cluster 2 has no member)
    mi_all = np.array([0.4, 0.3, 0.0, -0.01])
    poly = np.array([[3, 1, 3], [0, 0, 0], [2, 3, 0], [3, 3, 3]], dtype=np.uint8)
    s = G.lineage_summary(mi, mi_all, poly, neff)
    assert np.allclose(s["mi_within"], [2.0 / 30, 0.0, 10.0 / 30, 3.0 / 30], rtol=0, atol=1e-15)
    assert abs(s["within_frac"][0] - (2.0 / 30) / 0.4) < 1e-15 and s["within_frac"][1] == 0.0 and np.isnan(s["within_frac"][2:]).all()
    assert s["n_poly"].tolist() == [2, 0, 1, 3]
    assert s["top_cluster"].tolist() == [0, -1, 1, 1] and s["top_cluster"].dtype == np.int64
    assert s["top_share"][0] == 1.0 and np.isnan(s["top_share"][1]) and s["top_share"][2] == 1.0 and abs(s["top_share"][3] - 2.0 / 3.0) < 1e-15
    ref = R.summary_columns(mi, mi_all, poly, neff)
    for k in s:
        assert np.allclose(s[k], ref[k], rtol=0, atol=1e-15, equal_nan=True), k


def test_the_package_exports_the_lineage_entry_points():
    import ldweaver_amd
    for name in ("sequence_clusters", "link_lineage_mi"):
        assert name in ldweaver_amd.__all__ and getattr(ldweaver_amd, name) is getattr(G, name)


def test_a_null_context_is_refused_with_a_message():
    lib = L.lib()
    th, lab, n = np.array([3], dtype=np.int32), np.zeros(4, dtype=np.int32), np.zeros(1, dtype=np.int32)
    assert lib.ldw_seq_clusters(None, L.ptr(th), 1, L.ptr(lab), L.ptr(n)) == L.LDW_ERR_ARG
    assert b"null context" in lib.ldw_last_error()
    a = np.zeros(1, dtype=np.int32)
    mi, poly, fb = np.zeros(1), np.zeros(1, dtype=np.uint8), C.c_int(0)
    assert lib.ldw_links_stratified(None, L.ptr(a), L.ptr(a), 1, L.ptr(lab), 1, L.ptr(mi), L.ptr(mi), L.ptr(poly), L.ptr(mi), None, None, C.byref(fb)) == L.LDW_ERR_ARG
    assert b"null context" in lib.ldw_last_error()
