"""CPU: the co-change scan's numpy statement (tests/cochange_scan_ref.py; include/ldweaver_amd.h 23) against plain double loops and against
pars_ref.cochanges, ``pick_min_co`` at its edges, the planted example, and the new entries' declarations."""
import numpy as np
import pytest

import cochange_scan_ref as CR
import pars_ref as R
from ldweaver_amd import _lib as L
from ldweaver_amd import parsimony as P


def loops(change, changes, idx, B, min_co, min_lift, min_len, pos, g, best_in):
    """The statement, pair by pair."""
    M = len(changes)
    hist = np.zeros(CR.BINS, dtype=np.uint64)
    best, nge = np.full(M, -1, dtype=np.int32), np.zeros(M, dtype=np.int64)
    partner = np.full(M, -1, dtype=np.int32)
    npairs = nq = 0
    rows = []
    for a in range(M):
        for b in range(a + 1, M):
            if min_len >= 0:
                x = float(pos[b]) - float(pos[a])
                d = x - np.floor(x / g) * g
                d = d + g if d < 0 else d
                d = d - g if d >= g else d
                if not (0.5 * g - abs(d - 0.5 * g) > min_len):
                    continue
            npairs += 1
            co = int(np.count_nonzero(change[a] & change[b]))
            if co * B < min_lift * int(changes[a]) * int(changes[b]):
                continue
            nq += 1
            hist[min(co, CR.BINS - 1)] += 1
            for me, other in ((a, b), (b, a)):
                best[me] = max(best[me], co)
                nge[me] += co >= min_co
                if best_in is not None and best_in[me] >= 0 and co == best_in[me] and (partner[me] < 0 or idx[other] < partner[me]):
                    partner[me] = idx[other]
            if co >= min_co:
                rows.append((int(idx[a]), int(idx[b]), co))
    return dict(hist=hist, best=best, nge=nge, npairs=npairs, n_qualifying=nq, rows=sorted(rows), partner=partner)


@pytest.mark.parametrize("M, nodes, density, min_co, min_lift, min_len", [
    (0, 9, 0.5, 0, 0, -1.0), (1, 9, 0.5, 0, 0, -1.0), (2, 9, 0.5, 0, 0, -1.0), (7, 40, 0.3, 1, 0, -1.0), (12, 70, 0.5, 3, 2, -1.0), (9, 33, 0.6, 2, 1, 15.0),
    (11, 65, 0.1, 0, 3, 0.0), (8, 32, 1.0, 0, 1, 40.0),
])
def test_the_reference_against_double_loops(M, nodes, density, min_co, min_lift, min_len):
    rng = np.random.default_rng(M * 100 + nodes)
    change = rng.random((M, nodes)) < density
    change[:, 0] = False
    changes = change.sum(axis=1).astype(np.int32)
    idx = np.sort(rng.choice(200, size=M, replace=False)).astype(np.int32)
    g = 100.0
    pos = rng.integers(1, 100, size=M).astype(np.int32)
    B = nodes - 1
    got = CR.scan(change, changes, B, min_co, min_lift, min_len, pos, g)
    want = loops(change, changes, idx, B, min_co, min_lift, min_len, pos, g, got["best"])
    for k in ("hist", "best", "nge"):
        assert np.array_equal(got[k], want[k]), k
    assert (got["npairs"], got["n_qualifying"]) == (want["npairs"], want["n_qualifying"]) and int(got["hist"].sum()) == got["n_qualifying"]
    lk = CR.links(change, changes, idx, B, min_co, min_lift, min_len, pos, g, got["best"])
    assert list(zip(*[x.tolist() for x in CR.sorted_links(lk)])) == want["rows"] and lk["count"] == len(want["rows"])
    assert np.array_equal(lk["partner"], want["partner"])
    assert np.all(lk["a"] < lk["b"])
    # bitmaps and back
    assert np.array_equal(CR.unpack_bits(CR.pack_bits(change))[:, :nodes], change)


def test_the_hist_cap_ties_and_the_circle():
    # co of 1023, 1024 and 1056 all land in bin 1023
    change = np.zeros((4, 1057), dtype=bool)
    change[0, 1:], change[1, 1:] = True, True              # co(0, 1) = 1056
    change[2, 1:1024] = True                               # co(0, 2) = co(1, 2) = 1023
    change[3, 1:1025] = True                               # co(0, 3) = 1024, co(2, 3) = 1023
    r = CR.scan(change, change.sum(axis=1), 1056)
    assert r["hist"][1023] == 6 and r["hist"].sum() == 6 and r["best"].tolist() == [1056, 1056, 1023, 1024]
    # a tie on co between two partners: the smaller SNP wins
    change = np.zeros((3, 10), dtype=bool)
    change[0, 1:5], change[1, 1:3], change[2, 3:5] = True, True, True
    r = CR.scan(change, change.sum(axis=1), 9)
    lk = CR.links(change, change.sum(axis=1), [5, 7, 9], 9, best_in=r["best"])
    assert r["best"].tolist() == [2, 2, 2] and lk["partner"].tolist() == [7, 5, 5]
    # the circle: exactly min_len is out, just beyond is in, the short way round may cross the origin
    assert CR.circ_len(95, 5, 100.0) == 10.0 and CR.circ_len(5, 95, 100.0) == 10.0 and CR.circ_len(30, 5, 100.0) == 25.0
    pos = np.array([5, 15, 16, 95])
    in_p, _ = CR.pair_sets(np.zeros((4, 4), dtype=np.int64), np.ones(4), 9, 0, 10.0, pos, 100.0)
    assert np.argwhere(in_p).tolist() == [[0, 2], [1, 3], [2, 3]]      # (0, 1) and (0, 3) lie at exactly 10


@pytest.mark.parametrize("gap_mode", (0, 1))
def test_co_against_pars_ref_cochanges_pair_by_pair(gap_mode):
    rng = np.random.default_rng(3 + gap_mode)
    states = R.random_alignment(rng, 30, 21)
    parent, tip_seq = R.random_tree(rng, list(range(21)), max_arity=4, p_unary=0.1)
    ref = R.parsimony(parent, tip_seq, states, gap_mode)
    co = CR.co_matrix(ref["change"])
    a, b = np.triu_indices(30, 1)
    ca, cb, cc = R.cochanges(ref["change"], a, b)
    assert np.array_equal(co[a, b], cc) and np.array_equal(np.diag(co), ref["score"]) and np.array_equal(ca, ref["score"][a])
    assert np.array_equal(CR.co_matrix(CR.unpack_bits(CR.pack_bits(ref["change"]))), co)


def test_pick_min_co_at_its_edges():
    h = np.zeros(1024, dtype=np.uint64)
    assert P.pick_min_co(h, 0) == 1 and P.pick_min_co(h, 10, floor=5) == 5             # an empty histogram: the floor
    h[1023] = 50
    assert P.pick_min_co(h, 49) == 1023 and P.pick_min_co(h, 50) == 1 and P.pick_min_co(h, 0) == 1023      # everything in the open last bin
    h = np.zeros(1024, dtype=np.uint64)
    h[0], h[1], h[2], h[3], h[7] = 1000, 100, 10, 5, 1
    assert [P.pick_min_co(h, t) for t in (0, 1, 5, 6, 15, 16, 115, 116, 5000)] == [8, 4, 4, 3, 3, 2, 2, 1, 1]
    assert P.pick_min_co(h, 5000, floor=0) == 0 and P.pick_min_co(h, 0, floor=9) == 9 and P.pick_min_co(h, 3, floor=2000) == 1023
    with pytest.raises(ValueError, match="1024"):
        P.pick_min_co(np.zeros(4096), 3)


def test_the_planted_example_has_one_pair_that_changed_together_more_than_once():
    parent, tip_seq, states = CR.planted_example()
    assert states.shape == (40, 64) and 0.02 < np.mean(states == 4) < 0.08
    ref = R.parsimony(parent, tip_seq, states, 0)
    B = len(parent) - 1
    co = CR.co_matrix(ref["change"])
    for i in range(10):
        for j in range(i + 1, 10):
            assert co[i, j] == 1, (i, j)                       # the lineage markers: one shared branch, once
    assert co[10, 11] == 4 and ref["score"][10] == 4 and ref["score"][11] == 4
    up = np.triu(co, 1)
    assert int((up >= 2).sum()) == 1 and co.shape == (40, 40)  # the only pair of 780
    sc = CR.tree_scan(ref["change"], ref["score"], B, min_changes=1, min_co=2)
    assert sc["npairs"] == len(sc["idx"]) * (len(sc["idx"]) - 1) // 2
    lk = CR.tree_links(ref["change"], ref["score"], B, min_changes=1, min_co=2, best_in=sc["best"])
    assert (lk["a"].tolist(), lk["b"].tolist(), lk["co"].tolist()) == ([10], [11], [4])
    assert lk["partner"][10] == 11 and lk["partner"][11] == 10 and sc["best"][10] == 4
    assert P.pick_min_co(sc["hist"], 1) == 2
    assert P.cochange_pvalue(B, 4, 4, 4) < 1e-6 < P.cochange_pvalue(B, 1, 1, 1)


def test_the_new_entries_are_declared_and_exported_from_the_package():
    import ldweaver_amd
    api, debug = set(L.declared_symbols("ldweaver_amd.h")), set(L.declared_symbols("ldweaver_amd_debug.h"))
    assert {"ldw_tree_cochange_scan", "ldw_tree_cochange_links"} <= api and {"ldw_debug_cochange_scan", "ldw_debug_cochange_links"} <= debug
    for name in ("cochange_scan", "CochangeScan", "pick_min_co"):
        assert name in ldweaver_amd.__all__ and getattr(ldweaver_amd, name) is getattr(P, name)
    lib = L.lib()
    assert lib.ldw_tree_cochange_scan(None, None, None, 0, 0, 1, 0, 0, -1.0, None, None, None, None, None) == L.LDW_ERR_ARG       # no context: refused, no GPU needed
    n = np.zeros(1, dtype=np.int64)
    assert lib.ldw_debug_cochange_links(None, None, 1, 0, None, None, None, 0.0, 1, 0, 0, -1.0, None, 0, None, None, None, n.ctypes.data_as(L.C.POINTER(L.C.c_int64)),
                                        None) == L.LDW_ERR_ARG
