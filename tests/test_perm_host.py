"""Host: the permutation test for links — the replicate orders of the numpy restatement tests/perm_ref.py (valid, label-preserving,
evenly spread), the planted example of tests/test_lineage_host.py under it, the host-side policy of ldweaver_amd/lineage.py with a stub engine, and
what the entry point refuses without a device."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import lineage_ref
import perm_ref as R
from ldweaver_amd import _lib as L
from ldweaver_amd import lineage as G
from ldweaver_amd.snpdat import SnpDat
from test_lineage_host import planted


def test_the_hash_on_arrays_is_the_statement_on_integers():
    rng = np.random.default_rng(2)
    for seed in (0, 1, 12345, (1 << 64) - 1):
        r, s = rng.integers(0, 1 << 24, 50), rng.integers(0, 70000, 50)
        got = R.hash40(seed, r, s)
        assert got.dtype == np.uint64 and int(got.max()) < 1 << 40
        assert got.tolist() == [R.hash40_int(seed, int(x), int(y)) for x, y in zip(r, s)]


@pytest.mark.parametrize("seed", (0, 1, 12345))
def test_every_order_is_a_label_preserving_permutation_of_the_first(seed):
    rng = np.random.default_rng(seed)
    N, Cn = 300, 9
    labels = rng.integers(-1, Cn, N)
    labels[labels == 4] = 5                                        # a label without a member
    labels[0] = labels[-1] = -1
    o0 = R.order0(labels)
    assert np.array_equal(labels[o0], np.sort(labels[labels >= 0])) and o0.dtype == np.int32
    for c in range(Cn):
        assert np.all(np.diff(o0[labels[o0] == c]) > 0)            # ascending sequence index inside a cluster
    ords = R.orders(labels, 40, seed)
    assert ords.shape == (40, len(o0)) and ords.dtype == np.int32
    for r in range(40):
        assert np.array_equal(np.sort(ords[r]), np.sort(o0)), r
        assert np.array_equal(labels[ords[r]], labels[o0]), r      # position p holds a sequence of order0[p]'s cluster
    assert len({ords[r].tobytes() for r in range(40)}) == 40
    assert np.array_equal(ords[:7], R.orders(labels, 7, seed))     # replicate r does not depend on how many there are
    if seed:
        assert not np.array_equal(ords, R.orders(labels, 40, 0))


def test_singletons_never_move_and_seventy_thousand_sequences_give_valid_permutations():
    ords = R.orders(np.arange(50)[::-1], 5, 3)
    assert np.array_equal(ords, np.tile(np.arange(50)[::-1], (5, 1)))
    labels = np.random.default_rng(4).integers(0, 5, 70000)
    big = R.orders(labels, 4, 12345)
    o0 = R.order0(labels)
    for r in range(4):
        assert np.array_equal(np.bincount(big[r], minlength=70000), np.ones(70000, dtype=np.int64)) and np.array_equal(labels[big[r]], labels[o0])


@pytest.mark.parametrize("seed", (0, 1, 12345))
def test_the_orders_of_a_cluster_of_three_and_of_two_come_up_evenly(seed):
    """6 000 replicates: each of the six orders of the 3-cluster within 880 .. 1 120 (4 sigma about 1 000), each of the two of the 2-cluster within
    2 850 .. 3 150."""
    B = 6000
    ords = R.orders(np.array([0, 0, 0, 1, 1]), B, seed)
    three, two = Counter(map(tuple, ords[:, :3].tolist())), Counter(map(tuple, ords[:, 3:].tolist()))
    print(seed, sorted(three.values()), sorted(two.values()))
    assert len(three) == 6 and set(map(frozenset, three)) == {frozenset((0, 1, 2))}
    assert len(two) == 2 and set(map(frozenset, two)) == {frozenset((3, 4))}
    assert all(880 <= n <= 1120 for n in three.values()), sorted(three.values())
    assert all(2850 <= n <= 3150 for n in two.values()), sorted(two.values())


def test_planted_lineage_markers_keep_their_table_and_a_coupled_pair_gets_a_small_p():
    st, lin = planted(np.random.default_rng(7))
    hdw = np.ones(st.shape[1])
    B = 999
    a, b = [0, 4], [1, 5]
    free = R.links_permuted(st, hdw, a, b, np.zeros(len(lin), dtype=np.int64), 1, B, 0)
    within = R.links_permuted(st, hdw, a, b, lin, 2, B, 0)
    ref = lineage_ref.links_stratified(st, hdw, a, b, lin, 2)
    assert free["frac_bits"] == 0 and free["P"] == within["P"] == 200
    assert np.array_equal(free["mi_obs"], ref["mi_all"]) and np.array_equal(within["mi_obs"], ref["mi_all"])
    assert np.array_equal(within["fixed_obs"], ref["fixed"].sum(axis=1))
    cf, cw = (G.permutation_columns(x["mi_obs"], x["n_ge"], x["null_max"], B) for x in (free, within))
    # lineage markers: no unrestricted replicate reaches the observed MI; within the lineages every replicate's table is the observed one
    assert cf["perm_ge"][0] == 0 and cf["perm_p"][0] == 1.0 / (1 + B) and cf["null_max"][0] < 0.1 < cf["mi_all"][0]
    assert cw["perm_ge"][0] == B and cw["perm_p"][0] == 1.0
    assert np.all(within["fixed"][0] == within["fixed_obs"][0]) and np.all(within["null"][0] == within["mi_obs"][0])
    # the pair coupled inside the lineages
    assert cw["perm_p"][1] <= 0.01 and cf["perm_p"][1] <= 0.01
    # a's marginal and b's marginal are those of the observed table in every replicate
    for res in (free, within):
        assert np.array_equal(res["fixed"].sum(axis=3), np.broadcast_to(res["fixed_obs"].sum(axis=2)[:, None, :], (2, B, 5)))
        assert np.array_equal(res["fixed"].sum(axis=2), np.broadcast_to(res["fixed_obs"].sum(axis=1)[:, None, :], (2, B, 5)))


def test_the_weight_stays_with_the_sequence_and_with_the_first_snp():
    """A cluster of two sequences with different weights and different b-states: where they swap, the cell of a's state and the OTHER b-state gets the
    first sequence's own weight."""
    st = np.array([[1, 1, 0, 0], [2, 3, 0, 2]], dtype=np.uint8)     # (the last sequence makes b's states 2 and 3 unlike: the two tables differ in MI)
    hdw = np.array([1.0, 0.25, 0.5, 0.0625])
    V, F = lineage_ref.quantise(hdw)
    res = R.links_permuted(st, hdw, [0], [1], [0, 0, 1, 2], 3, 64, 5)
    swapped = res["orders"][:, 0] == 1
    assert swapped.any() and not swapped.all()
    for r in range(64):
        want = np.zeros((5, 5), dtype=np.int64)
        want[0, 0], want[0, 2] = V[2], V[3]
        if swapped[r]:
            want[1, 3], want[1, 2] = V[0], V[1]
        else:
            want[1, 2], want[1, 3] = V[0], V[1]
        assert np.array_equal(res["fixed"][0, r], want), r
    assert np.array_equal(res["fixed"][0][~swapped][0], res["fixed_obs"][0]) and len(np.unique(res["null"][0])) == 2


def test_permutation_columns():
    c = G.permutation_columns([0.5, 0.0, 0.25], np.array([0, 999, 9], dtype=np.int32), [0.1, 0.0, 0.3], 999)
    assert list(c) == ["mi_all", "perm_ge", "perm_p", "null_max", "n_perm"]
    assert c["perm_p"].tolist() == [1.0 / 1000, 1.0, 10.0 / 1000] and c["perm_ge"].dtype == np.int64 and c["perm_ge"].tolist() == [0, 999, 9]
    assert c["n_perm"].tolist() == [999] * 3 and c["n_perm"].dtype == np.int64 and c["mi_all"].tolist() == [0.5, 0.0, 0.25] and c["null_max"].tolist() == [0.1, 0.0, 0.3]
    assert all(len(v) == 0 for v in G.permutation_columns([], [], [], 10).values())
    for bad in (([0.1], [11], [0.1], 10), ([0.1], [-1], [0.1], 10), ([0.1], [0], [0.1], 0)):
        with pytest.raises(ValueError):
            G.permutation_columns(*bad)


class StubEngine:
    """What link_permutation_test asks of an engine, answered from tests/perm_ref.py."""

    def __init__(self, states):
        self.states, (self.L, self.N) = states, states.shape
        self.calls, self.hdw = [], None

    def hamming_weights(self, thresh):
        self.calls.append(("hamming_weights", thresh))
        return np.full(self.N, 0.5)

    def set_weights(self, hdw):
        self.hdw = np.asarray(hdw, dtype=np.float64)

    def links_permuted(self, a, b, labels, n_perm, seed=0, C=None, want_null=False, want_tables=False, want_orders=False):
        self.calls.append(("links_permuted", np.asarray(a).tolist(), np.asarray(b).tolist(), np.asarray(labels).tolist(), n_perm, seed, C, want_null))
        res = R.links_permuted(self.states, self.hdw, a, b, labels, C, n_perm, seed)
        out = {k: res[k] for k in ("mi_obs", "n_ge", "null_max")}
        if want_null:
            out["null"] = res["null"]
        return out

    def close(self):
        raise AssertionError("a caller's engine is not closed")


def test_link_permutation_test_appends_its_columns_and_passes_the_clusters_on(tmp_path):
    import pandas as pd
    st, lin = planted(np.random.default_rng(7), n_per=20)
    names = [f"s{k}" for k in range(40)]
    snp = SnpDat.from_states(st, np.array([10, 20, 30, 40, 50, 60]), 100.0, seq_names=names)
    links = pd.DataFrame({"pos1": [50, 10, 10], "pos2": [60, 20, 20], "MI": [0.3, 0.2, 0.1]}, index=[7, 8, 9])
    eng = StubEngine(st)
    out = tmp_path / "perm.tsv"
    df, null = G.link_permutation_test(links, None, snp, n_perm=50, seed=3, engine=eng, alignment_resident=True, return_null=True, out_path=out)
    assert eng.calls == [("hamming_weights", 0), ("links_permuted", [4, 0, 0], [5, 1, 1], [0] * 40, 50, 3, 1, True)]
    assert list(df.columns) == ["pos1", "pos2", "MI", "mi_all", "perm_ge", "perm_p", "null_max", "n_perm"] and list(df.index) == [7, 8, 9]
    assert df["MI"].tolist() == [0.3, 0.2, 0.1] and "mi_all" not in links.columns and null.shape == (3, 50)
    ref = R.links_permuted(st, np.full(40, 0.5), [4, 0, 0], [5, 1, 1], np.zeros(40, dtype=np.int64), 1, 50, 3)
    assert np.array_equal(df["mi_all"], ref["mi_obs"]) and np.array_equal(df["perm_ge"], ref["n_ge"]) and np.array_equal(null, ref["null"])
    assert np.array_equal(df["perm_p"], (1.0 + ref["n_ge"]) / 51.0) and df["n_perm"].tolist() == [50] * 3
    assert df["perm_ge"].tolist()[1:] == [0, 0] and df.iloc[1, 3:].tolist() == df.iloc[2, 3:].tolist()       # a repeated link: equal rows
    back = pd.read_csv(out, sep="\t")
    assert list(back.columns) == list(df.columns) and len(back) == 3 and np.allclose(back["perm_p"], df["perm_p"], rtol=1e-12, atol=0)
    # clusters by name, given weights, no null back: lineage markers get p = 1
    eng.calls.clear()
    clusters = pd.Series(np.where(lin == 0, "x", "y")[::-1], index=names[::-1])
    hdw = 1.0 / (1.0 + np.arange(40) % 3)
    df2 = G.link_permutation_test(links, clusters, snp, n_perm=20, hdw=hdw, engine=eng, alignment_resident=True)
    assert eng.calls == [("links_permuted", [4, 0, 0], [5, 1, 1], lin.tolist(), 20, 0, 2, False)] and np.array_equal(eng.hdw, hdw)
    assert df2["perm_p"].tolist()[1:] == [1.0, 1.0] and df2["perm_ge"].tolist()[1:] == [20, 20]
    # no links: the columns, no call
    eng.calls.clear()
    empty = G.link_permutation_test(links.iloc[:0], lin, snp, n_perm=20, hdw=hdw, engine=eng, alignment_resident=True)
    assert len(empty) == 0 and list(empty.columns) == list(df.columns) and eng.calls == []
    for bad in (dict(n_perm=0), dict(n_perm=(1 << 24) + 1)):
        with pytest.raises(ValueError):
            G.link_permutation_test(links, lin, snp, engine=eng, alignment_resident=True, **bad)
    with pytest.raises(ValueError):
        G.link_permutation_test(links, lin[:-1], snp, engine=eng, alignment_resident=True)
    with pytest.raises(ValueError):
        G.link_permutation_test(links.assign(pos1=[11, 10, 10]), lin, snp, engine=eng, alignment_resident=True)


def test_the_package_exports_the_permutation_test_and_the_library_its_entry_point():
    import ldweaver_amd
    assert "link_permutation_test" in ldweaver_amd.__all__ and ldweaver_amd.link_permutation_test is G.link_permutation_test
    assert "ldw_links_permuted" in L.declared_symbols() and hasattr(L.lib(), "ldw_links_permuted")


def test_a_null_context_is_refused_with_a_message():
    lib = L.lib()
    a, lab = np.zeros(1, dtype=np.int32), np.zeros(4, dtype=np.int32)
    mi, n_ge, p, fb = np.zeros(1), np.zeros(1, dtype=np.int32), C.c_int64(0), C.c_int(0)
    rc = lib.ldw_links_permuted(None, L.ptr(a), L.ptr(a), 1, L.ptr(lab), 1, 10, 0, L.ptr(mi), L.ptr(n_ge), L.ptr(mi), None, None, None, C.byref(p), C.byref(fb))
    assert rc == L.LDW_ERR_ARG and b"null context" in lib.ldw_last_error()
