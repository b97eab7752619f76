"""GPU: the co-change scan through the tree (ldw_tree_cochange_scan, ldw_tree_cochange_links, parsimony.cochange_scan; pytest -m gpu) against
pars_ref.parsimony + the numpy statement tests/cochange_scan_ref.py.  Everything compared is an integer and every comparison is array_equal; lists are
compared after a lexsort."""
import ctypes as C

import numpy as np
import pytest

import cochange_scan_ref as CR
import pars_ref as R
from ldweaver_amd import _lib as L
from ldweaver_amd import parsimony as P
from ldweaver_amd.engine import Engine
from ldweaver_amd.snpdat import SnpDat
from ldweaver_amd.tree import Tree

pytestmark = pytest.mark.gpu


def check(eng, parent, tip_seq, states, gap_mode, min_changes=2, min_co=2, min_lift=0, min_len=-1.0, POS=None, g=None, ref=None, tag=None):
    """Both entries on the alignment the engine holds against the reference, and every listed pair against ldw_tree_cochanges; returns (reference scan,
    device links)."""
    ref = R.parsimony(parent, tip_seq, states, gap_mode) if ref is None else ref
    B = len(parent) - 1
    kw = dict(min_changes=min_changes, min_co=min_co, min_lift=min_lift, min_len=min_len)
    want = CR.tree_scan(ref["change"], ref["score"], B, POS=POS, g=g, **kw)
    got = eng.tree_cochange_scan(parent, tip_seq, gap_mode, **kw)
    for k in ("changes", "hist", "best", "nge"):
        assert np.array_equal(got[k], want[k]), (tag, k)
    assert (got["npairs"], got["n_qualifying"]) == (want["npairs"], want["n_qualifying"]) and int(got["hist"].sum()) == got["n_qualifying"], tag
    wl = CR.tree_links(ref["change"], ref["score"], B, POS=POS, g=g, best_in=want["best"], **kw)
    n = eng.tree_cochange_links(parent, tip_seq, gap_mode, **kw)["count"]
    assert n == wl["count"], tag
    lk = eng.tree_cochange_links(parent, tip_seq, gap_mode, cap=n, best_in=got["best"], **kw)
    assert lk["count"] == n and np.array_equal(lk["partner"], wl["partner"]), (tag, "partner")
    if n:
        a, b, co = CR.sorted_links(lk)
        assert all(np.array_equal(x, y) for x, y in zip((a, b, co), CR.sorted_links(wl))), (tag, "lists")
        ca, cb, cc = eng.tree_cochanges(parent, tip_seq, a, b, gap_mode)          # the parent's only route to the same integers
        assert np.array_equal(cc, co) and np.array_equal(ca, got["changes"][a]) and np.array_equal(cb, got["changes"][b]), (tag, "ldw_tree_cochanges")
    return want, lk


@pytest.mark.parametrize("Ls", (65, 257))
@pytest.mark.parametrize("n", (2, 17, 65, 200))
def test_shapes_on_a_caterpillar_a_balanced_tree_and_random_polytomies_with_unary_nodes(engine, n, Ls):
    rng = np.random.default_rng(1000 * n + Ls)
    states = R.random_alignment(rng, Ls, n)
    engine.set_alignment(states)
    seqs = list(range(n))
    trees = dict(caterpillar=R.caterpillar(seqs), balanced=R.balanced(seqs), polytomies=R.random_tree(rng, rng.permutation(n).tolist(), max_arity=6, p_unary=0.2))
    for name, (parent, tip_seq) in trees.items():
        for gap_mode in (0, 1):
            ref = R.parsimony(parent, tip_seq, states, gap_mode)
            check(engine, parent, tip_seq, states, gap_mode, min_changes=1, min_co=1, ref=ref, tag=(name, gap_mode, "all"))
            check(engine, parent, tip_seq, states, gap_mode, min_changes=2, min_co=2, min_lift=1, ref=ref, tag=(name, gap_mode, "lift"))


@pytest.mark.parametrize("nodes", (31, 32, 33, 65))
def test_node_counts_on_both_sides_of_a_bitmap_word(engine, nodes):
    rng = np.random.default_rng(nodes)
    n = (nodes + 1) // 2 if nodes & 1 else nodes // 2
    parent, tip_seq = R.caterpillar(list(range(n)))
    if not nodes & 1:                                   # a unary node on top of the caterpillar
        parent = np.concatenate([[-1, 0], parent[1:] + 1]).astype(np.int32)
        tip_seq = np.concatenate([[-1], tip_seq]).astype(np.int32)
    assert len(parent) == nodes
    states = R.random_alignment(rng, 130, n)
    engine.set_alignment(states)
    for gap_mode in (0, 1):
        check(engine, parent, tip_seq, states, gap_mode, min_changes=1, min_co=2, tag=(nodes, gap_mode))


def test_a_tree_over_a_subset_of_the_sequences_and_min_len_on_the_snp_positions(engine):
    rng = np.random.default_rng(77)
    states = R.random_alignment(rng, 130, 66)
    engine.set_alignment(states)
    POS = np.sort(rng.choice(np.arange(1, 3000), size=130, replace=False)).astype(np.int32)
    half = rng.permutation(66)[:33].tolist()
    parent, tip_seq = R.random_tree(rng, half, max_arity=4, p_unary=0.1)
    with pytest.raises(L.LdwError, match="needs the SNP positions") as e:        # the alignment is new: no positions yet
        engine.tree_cochange_scan(parent, tip_seq, 0, min_len=10.0)
    assert e.value.code == L.LDW_ERR_STATE
    engine.set_snp_meta(np.ones(130), np.ones((130, 5)), POS, None, 3000.0)
    for gap_mode in (0, 1):
        check(engine, parent, tip_seq, states, gap_mode, min_changes=2, min_co=3, tag=("half", gap_mode))
        want, _ = check(engine, parent, tip_seq, states, gap_mode, min_changes=2, min_co=3, min_lift=1, min_len=400.0, POS=POS, g=3000.0, tag=("half, len", gap_mode))
        full = CR.tree_scan(R.parsimony(parent, tip_seq, states, gap_mode)["change"], want["changes"], len(parent) - 1, min_changes=2)
        assert 0 < want["npairs"] < full["npairs"]


def test_min_changes_one_two_and_above_every_score(engine):
    rng = np.random.default_rng(8)
    states = R.random_alignment(rng, 90, 40)
    engine.set_alignment(states)
    parent, tip_seq = R.balanced(list(range(40)))
    ref = R.parsimony(parent, tip_seq, states, 0)
    m1, _ = check(engine, parent, tip_seq, states, 0, min_changes=1, min_co=4, ref=ref)
    m2, _ = check(engine, parent, tip_seq, states, 0, min_changes=2, min_co=4, ref=ref)
    assert len(m1["idx"]) == int((ref["score"] >= 1).sum()) < 90 and len(m2["idx"]) <= len(m1["idx"])       # (the constant column and the all-N column never change)
    top = int(ref["score"].max())
    one, lk = check(engine, parent, tip_seq, states, 0, min_changes=top, min_co=0, ref=ref)                   # M >= 1
    none, lk0 = check(engine, parent, tip_seq, states, 0, min_changes=top + 1, min_co=0, ref=ref)             # M = 0
    assert none["npairs"] == 0 and np.all(none["best"] == -1) and lk0["count"] == 0 and np.all(lk0["partner"] == -1) and none["hist"].sum() == 0
    assert one["npairs"] == len(one["idx"]) * (len(one["idx"]) - 1) // 2


def test_forced_chunks_of_the_passes_give_the_results_of_the_default(engine, monkeypatch):
    rng = np.random.default_rng(9)
    states = R.random_alignment(rng, 600, 33, p_n=0.1)
    engine.set_alignment(states)
    parent, tip_seq = R.random_tree(rng, list(range(33)), max_arity=5, p_unary=0.1)
    ref = R.parsimony(parent, tip_seq, states, 0)
    monkeypatch.delenv("LDW_PARS_CHUNK", raising=False)
    want, want_l = check(engine, parent, tip_seq, states, 0, min_changes=2, min_co=9, min_lift=1, ref=ref, tag="default")
    assert len(want["idx"]) > 2 * 256 and want_l["count"] > 10                   # more than two chunks of eligible SNPs
    monkeypatch.setenv("LDW_PARS_CHUNK", "256")
    got, got_l = check(engine, parent, tip_seq, states, 0, min_changes=2, min_co=9, min_lift=1, ref=ref, tag="chunks of 256")
    assert all(np.array_equal(x, y) for x, y in zip(CR.sorted_links(got_l), CR.sorted_links(want_l)))


def test_the_context_keeps_its_alignment_and_the_timing_slots_add_up(engine):
    rng = np.random.default_rng(13)
    states = R.random_alignment(rng, 130, 64)
    engine.set_alignment(states)
    before = (engine.get_alignment().tobytes(), engine.hamming_weights(13).tobytes())
    parent, tip_seq = R.balanced(list(range(64)))
    for call in (lambda: engine.tree_cochange_scan(parent, tip_seq, 0), lambda: engine.tree_cochange_links(parent, tip_seq, 0, cap=0)):
        call()
        ms = np.zeros(4)
        assert L.lib().ldw_ctx_last_timing(engine._ctx, L.ptr(ms)) == L.LDW_OK
        assert np.all(ms[:3] >= 0) and ms[0] > 0 and ms[1] > 0 and abs(ms[3] - ms[:3].sum()) < 1e-9
    assert (engine.get_alignment().tobytes(), engine.hamming_weights(13).tobytes()) == before


def test_the_planted_example_end_to_end_through_cochange_scan(engine, tmp_path):
    import pandas as pd
    parent, tip_seq, states = CR.planted_example()
    names = [f"iso{k}" for k in range(64)]
    POS = (np.arange(40, dtype=np.int32) * 50 + 7)
    snp = SnpDat.from_states(states, POS, 4000, seq_names=names)
    # the Tree of the same topology: the tips of pars_ref.balanced carry the sequences 0..63 in order
    tips = np.flatnonzero(tip_seq >= 0)
    kids = R.children_of(parent)
    tree = Tree(parent=np.asarray(parent, dtype=np.int32), length=np.ones(len(parent)), tip_label=[names[int(tip_seq[v])] for v in tips], tip_node=tips.astype(np.int32),
                child_ptr=np.concatenate([[0], np.cumsum([len(k) for k in kids])]).astype(np.int32), child_idx=np.array([u for k in kids for u in k], dtype=np.int32))
    out = tmp_path / "cochange.tsv"
    res = P.cochange_scan(tree, snp, engine=engine, min_changes=1, min_co=2, out_path=out)
    assert isinstance(res, P.CochangeScan) and res.min_co == 2 and res.npairs == len(res.snps[res.snps["changes"] >= 1]) * (len(res.snps[res.snps["changes"] >= 1]) - 1) // 2
    assert list(res.links.columns) == ["pos1", "pos2", "len", "changes1", "changes2", "co_changes", "co_p", "jaccard"]
    assert len(res.links) == 1 and res.links.loc[0, ["pos1", "pos2", "changes1", "changes2", "co_changes"]].tolist() == [POS[10], POS[11], 4, 4, 4]
    assert res.links.loc[0, "co_p"] == P.cochange_pvalue(len(parent) - 1, 4, 4, 4) and res.links.loc[0, "jaccard"] == 1.0 and res.links.loc[0, "len"] == 50.0
    assert list(res.snps.columns) == ["POS", "changes", "best_co", "best_partner", "n_partners"]
    assert res.snps.loc[10, "best_partner"] == POS[11] and res.snps.loc[11, "best_partner"] == POS[10] and res.snps.loc[10, "best_co"] == 4
    assert res.snps.loc[10, "n_partners"] == 1 and int(res.snps["n_partners"].sum()) == 2
    ref = R.parsimony(parent, tip_seq, states, 0)
    want = CR.tree_scan(ref["change"], ref["score"], len(parent) - 1, min_changes=1, min_co=2)
    assert np.array_equal(res.hist, want["hist"]) and np.array_equal(res.snps["best_co"], want["best"]) and res.n_qualifying == want["n_qualifying"]
    for i in range(10):
        assert res.snps.loc[i, "best_co"] == 1                                     # a lineage marker shares its one branch, once
    back = pd.read_csv(out, sep="\t")
    assert list(back.columns) == list(res.links.columns) and back.loc[0, "co_changes"] == 4
    # with top: the cut rises until at most `top` pairs are listed; the partners are counted at the cut used
    top = P.cochange_scan(tree, snp, engine=engine, alignment_resident=True, min_changes=1, min_co=0, top=50)
    assert top.min_co == P.pick_min_co(want["hist"], 50, floor=0) >= 1 and len(top.links) == int(want["hist"][top.min_co:].sum()) <= 50
    assert np.array_equal(top.links["co_p"], np.sort(top.links["co_p"])) and int(top.snps["n_partners"].sum()) == 2 * len(top.links)
    far = P.cochange_scan(tree, snp, engine=engine, min_changes=1, min_co=2, min_len=60)
    assert len(far.links) == 0 and far.npairs < res.npairs                    # the planted pair lies 50 apart
    with pytest.raises(ValueError, match="min_len needs"):
        P.cochange_scan(tree, None, engine=engine, alignment_resident=True, min_len=5)


def test_every_refusal_names_its_cause_and_leaves_the_context_working(engine):
    rng = np.random.default_rng(17)
    states = R.random_alignment(rng, 20, 9)
    parent, tip_seq = R.balanced(list(range(8)))
    nodes = len(parent)
    with Engine(0) as fresh:                              # no alignment resident
        for call in (lambda: fresh.tree_cochange_scan(parent, tip_seq), lambda: fresh.tree_cochange_links(parent, tip_seq)):
            with pytest.raises(L.LdwError, match="no alignment resident") as e:
                call()
            assert e.value.code == L.LDW_ERR_STATE
    engine.set_alignment(states)
    ref = R.parsimony(parent, tip_seq, states, 0)

    def good():
        check(engine, parent, tip_seq, states, 0, min_changes=1, min_co=1, ref=ref)

    def changed(arr, at, value):
        out = arr.copy()
        out[at] = value
        return out

    tips = np.flatnonzero(tip_seq >= 0)
    bad = [
        (dict(parent=changed(parent, 0, 0)), r"parent\[0\] = 0"), (dict(parent=changed(parent, 5, 9)), r"parent\[5\] = 9"),
        (dict(tip_seq=changed(tip_seq, tips[2], 9)), f"tip node {tips[2]} names sequence 9"), (dict(gap_mode=2), "gap_mode 2"),
        (dict(min_changes=0), "min_changes 0"), (dict(min_co=-1), "min_co -1"), (dict(min_lift=-1), "min_lift -1"), (dict(min_lift=2 ** 20 + 1), "min_lift 1048577"),
        (dict(min_len=np.nan), "min_len is NaN"),
    ]
    for kw, msg in bad:
        args = dict(parent=parent, tip_seq=tip_seq, gap_mode=0)
        args.update(kw)
        for call in (engine.tree_cochange_scan, engine.tree_cochange_links):
            with pytest.raises(L.LdwError, match=msg) as e:
                call(**args)
            assert e.value.code == L.LDW_ERR_ARG and call.__name__[5:] in str(e.value), msg
        good()
    with pytest.raises(L.LdwError, match="needs the SNP positions") as e:
        engine.tree_cochange_links(parent, tip_seq, 0, min_len=0.0)
    assert e.value.code == L.LDW_ERR_STATE
    K = 2 ** 21 - 1                                       # a chain of K unary nodes with two tips under the last: 2^21 + 1 nodes, a legal tree of (17)
    big = np.concatenate([np.arange(-1, K - 1), [K - 1, K - 1]]).astype(np.int32)
    big_tips = np.concatenate([np.full(K, -1), [0, 1]]).astype(np.int32)
    with pytest.raises(L.LdwError, match=r"2097153 nodes \(at most 2\^21\)") as e:
        engine.tree_cochange_scan(big, big_tips, 0)
    assert e.value.code == L.LDW_ERR_ARG
    lib, n = L.lib(), C.c_int64(0)
    out, h = np.zeros(20, dtype=np.int32), np.zeros(1024, dtype=np.uint64)
    o64, np2 = np.zeros(20, dtype=np.int64), np.zeros(2, dtype=np.int64)
    tree = (engine._ctx, L.ptr(parent), L.ptr(tip_seq), nodes, 0, 1, 0, 0, -1.0)
    assert lib.ldw_tree_cochange_scan(*tree, None, L.ptr(h), L.ptr(out), L.ptr(o64), L.ptr(np2)) == L.LDW_ERR_ARG and b"output is null" in lib.ldw_last_error()
    assert lib.ldw_tree_cochange_scan(*tree, L.ptr(out), L.ptr(h), L.ptr(out), L.ptr(o64), None) == L.LDW_ERR_ARG
    assert lib.ldw_tree_cochange_links(*tree, None, 0, None, None, None, C.byref(n), L.ptr(out)) == L.LDW_ERR_ARG and b"partner_out needs best_in" in lib.ldw_last_error()
    assert lib.ldw_tree_cochange_links(*tree, None, 0, None, None, None, None, None) == L.LDW_ERR_ARG and b"null count_out" in lib.ldw_last_error()
    assert lib.ldw_tree_cochange_links(*tree, None, 3, L.ptr(out), None, L.ptr(out), C.byref(n), None) == L.LDW_ERR_ARG
    with pytest.raises(L.LdwError) as e:
        engine.tree_cochange_links(parent, tip_seq, 0, min_changes=1, min_co=0, cap=1)
    assert e.value.code == L.LDW_ERR_SIZE and e.value.count == CR.tree_links(ref["change"], ref["score"], nodes - 1, min_changes=1, min_co=0)["count"] > 1
    good()
