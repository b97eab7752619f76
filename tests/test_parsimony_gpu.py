"""GPU: parsimony on a tree (ldw_tree_parsimony, ldw_tree_states, ldw_tree_cochanges) against the numpy restatement tests/pars_ref.py
(pytest -m gpu).  Everything compared is an integer and every comparison is array_equal."""
import numpy as np
import pytest

import caller_stream_job as J
import pars_ref as R
from ldweaver_amd import _lib as L
from ldweaver_amd import parsimony as P
from ldweaver_amd.engine import Engine
from ldweaver_amd.snpdat import SnpDat
from ldweaver_amd.tree import tree_from_joins

pytestmark = pytest.mark.gpu

TIPS = (2, 3, 4, 17, 33, 64, 65, 200)
COLUMNS = (1, 63, 64, 65, 130, 257)


def some_pairs(rng, L, K):
    """K pairs among L SNPs; where K allows, the first is a == b and the last two are one pair twice."""
    a, b = rng.integers(0, L, size=K).astype(np.int32), rng.integers(0, L, size=K).astype(np.int32)
    b[0] = a[0]
    if K >= 3:
        a[-1], b[-1] = a[-2], b[-2]
    return a, b


def check(eng, parent, tip_seq, states, gap_mode, rng, ref=None, n_pairs=40, tag=None):
    """The three entry points on the alignment the engine holds, against the reference: scores and min_changes of all SNPs; the states of all SNPs in
    a shuffled order with one listed twice; pairs; a SNP's changes are its score."""
    ref = R.parsimony(parent, tip_seq, states, gap_mode) if ref is None else ref
    Ls = states.shape[0]
    score, mn = eng.tree_parsimony(parent, tip_seq, gap_mode)
    assert np.array_equal(score, ref["score"]), (tag, "score")
    assert np.array_equal(mn, ref["min_changes"]), (tag, "min_changes")
    idx = np.concatenate([rng.permutation(Ls), [int(rng.integers(Ls))]]).astype(np.int32)
    st = eng.tree_states(parent, tip_seq, idx, gap_mode)
    assert st.shape == (Ls + 1, len(parent)) and np.array_equal(st, ref["state"][idx]), (tag, "states")
    a, b = some_pairs(rng, Ls, n_pairs)
    ca, cb, co = eng.tree_cochanges(parent, tip_seq, a, b, gap_mode)
    ra, rb, rco = R.cochanges(ref["change"], a, b)
    assert np.array_equal(ca, ra) and np.array_equal(cb, rb) and np.array_equal(co, rco), (tag, "pairs")
    assert np.array_equal(ca, ref["score"][a]) and np.array_equal(cb, ref["score"][b]) and co[0] == ca[0], (tag, "changes = score")
    return ref


@pytest.mark.parametrize("Ls", COLUMNS)
@pytest.mark.parametrize("n", TIPS)
def test_shapes_on_a_caterpillar_a_balanced_tree_and_random_polytomies_with_unary_nodes(engine, n, Ls):
    rng = np.random.default_rng(1000 * n + Ls)
    states = R.random_alignment(rng, Ls, n)
    engine.set_alignment(states)
    seqs = list(range(n))
    trees = dict(caterpillar=R.caterpillar(seqs), balanced=R.balanced(seqs), polytomies=R.random_tree(rng, rng.permutation(n).tolist(), max_arity=6, p_unary=0.2))
    for name, (parent, tip_seq) in trees.items():
        for gap_mode in (0, 1):
            check(engine, parent, tip_seq, states, gap_mode, rng, tag=(name, gap_mode))


@pytest.mark.parametrize("nodes", (31, 32, 33, 63, 64, 65, 96, 97))
def test_node_counts_on_both_sides_of_a_bitmap_word(engine, nodes):
    """A caterpillar (an odd number of nodes), with a unary node on top of it where the count is even: the last word of a SNP's bitmap of changed
    branches holds 31, 32 and 1 bits."""
    rng = np.random.default_rng(nodes)
    n = (nodes + 1) // 2 if nodes & 1 else nodes // 2
    parent, tip_seq = R.caterpillar(list(range(n)))
    if not nodes & 1:
        parent = np.concatenate([[-1, 0], parent[1:] + 1]).astype(np.int32)
        tip_seq = np.concatenate([[-1], tip_seq]).astype(np.int32)
    assert len(parent) == nodes
    states = R.random_alignment(rng, 65, n)
    engine.set_alignment(states)
    for gap_mode in (0, 1):
        check(engine, parent, tip_seq, states, gap_mode, rng, tag=(nodes, gap_mode))


def test_a_star_of_300_tips_counts_past_255(engine):
    rng = np.random.default_rng(300)
    states = R.random_alignment(rng, 65, 300)
    states[3] = 0
    states[3, :3] = 1                                   # 297 children agree: K = 297
    states[4] = np.where(np.arange(300) < 256, 2, 3)    # K = 256: what 8 bits would wrap to 0
    engine.set_alignment(states)
    parent, tip_seq = R.star(rng.permutation(300).tolist())
    for gap_mode in (0, 1):
        ref = check(engine, parent, tip_seq, states, gap_mode, rng, tag=("star", gap_mode))
        assert ref["score"][3] == 3 and ref["score"][4] == 44
    # the star as one child of a binary root beside a tip: arity 299 below arity 2
    parent2 = np.concatenate([[-1, 0], np.full(299, 1), [0]]).astype(np.int32)
    tip_seq2 = np.concatenate([[-1, -1], rng.permutation(300)]).astype(np.int32)
    check(engine, parent2, tip_seq2, states, 0, rng, tag="star under a root")


def test_the_nj_tree_of_the_same_alignment_and_a_tree_on_half_of_the_sequences(engine):
    rng = np.random.default_rng(77)
    states = R.random_alignment(rng, 130, 66)
    engine.set_alignment(states)
    par, ln = engine.nj_tree()
    parent, tip_seq = R.from_tree(tree_from_joins(par, ln))
    assert np.bincount(parent[1:]).max() == 3
    for gap_mode in (0, 1):
        check(engine, parent, tip_seq, states, gap_mode, rng, tag=("nj", gap_mode))
    half = rng.permutation(66)[:33].tolist()
    for make in (R.balanced, lambda s: R.random_tree(rng, s, max_arity=4, p_unary=0.1)):
        parent, tip_seq = make(half)
        for gap_mode in (0, 1):
            ref = check(engine, parent, tip_seq, states, gap_mode, rng, tag=("half", gap_mode))
            sub = R.parsimony(*R.finish(parent, list(range(33))), np.ascontiguousarray(states[:, tip_seq[tip_seq >= 0]]), gap_mode)
            assert np.array_equal(ref["score"], sub["score"]) and np.array_equal(ref["min_changes"], sub["min_changes"])


def test_special_columns(engine):
    """A constant column, an all-N column, a column of one state plus N: score, min_changes and states under both gap modes, stated outright."""
    rng = np.random.default_rng(5)
    states = R.random_alignment(rng, 8, 40)
    assert np.all(states[0] == 2) and np.all(states[1] == 4) and set(states[2].tolist()) == {1, 4}
    engine.set_alignment(states)
    parent, tip_seq = R.balanced(list(range(40)))
    for gap_mode in (0, 1):
        check(engine, parent, tip_seq, states, gap_mode, rng)
    score, mn = engine.tree_parsimony(parent, tip_seq, 0)
    assert score[:3].tolist() == [0, 0, 0] and mn[:3].tolist() == [0, 0, 0]
    st = engine.tree_states(parent, tip_seq, [0, 1, 2], 0)
    assert np.all(st[0] == 2) and np.all(st[1] == 0) and np.all(st[2] == 1)
    score, mn = engine.tree_parsimony(parent, tip_seq, 1)
    assert score[:2].tolist() == [0, 0] and mn[:3].tolist() == [0, 0, 1] and score[2] >= 1
    st = engine.tree_states(parent, tip_seq, [1], 1)
    assert np.all(st == 4)


@pytest.mark.parametrize("chunk", ("1", "64", "100"))
def test_forced_chunks_give_the_results_of_the_default(engine, monkeypatch, chunk):
    rng = np.random.default_rng(9)
    states = R.random_alignment(rng, 257, 33)
    engine.set_alignment(states)
    parent, tip_seq = R.random_tree(rng, list(range(33)), max_arity=5, p_unary=0.1)
    idx = rng.permutation(257).astype(np.int32)
    a, b = some_pairs(rng, 257, 400)                    # about 250 distinct SNPs: more than a chunk of 1, 64 or 100 holds
    assert len(np.unique(np.concatenate([a, b]))) > 200
    monkeypatch.delenv("LDW_PARS_CHUNK", raising=False)
    want = (engine.tree_parsimony(parent, tip_seq, 0), engine.tree_states(parent, tip_seq, idx, 0), engine.tree_cochanges(parent, tip_seq, a, b, 0))
    ref = R.parsimony(parent, tip_seq, states, 0)
    assert np.array_equal(want[0][0], ref["score"]) and np.array_equal(want[1], ref["state"][idx])
    assert all(np.array_equal(x, y) for x, y in zip(want[2], R.cochanges(ref["change"], a, b)))
    monkeypatch.setenv("LDW_PARS_CHUNK", chunk)
    got = (engine.tree_parsimony(parent, tip_seq, 0), engine.tree_states(parent, tip_seq, idx, 0), engine.tree_cochanges(parent, tip_seq, a, b, 0))
    assert np.array_equal(got[0][0], want[0][0]) and np.array_equal(got[0][1], want[0][1])
    assert np.array_equal(got[1], want[1])
    assert all(np.array_equal(x, y) for x, y in zip(got[2], want[2]))


def test_pairs_one_pair_a_thousand_pairs_over_three_snps_and_repeats(engine):
    rng = np.random.default_rng(11)
    states = R.random_alignment(rng, 130, 65)
    engine.set_alignment(states)
    parent, tip_seq = R.random_tree(rng, list(range(65)), max_arity=3)
    ref = R.parsimony(parent, tip_seq, states, 0)
    for a, b in (([7], [93]), ([5], [5]), ([3, 3, 129], [60, 60, 0])):
        got = engine.tree_cochanges(parent, tip_seq, a, b, 0)
        assert all(np.array_equal(x, y) for x, y in zip(got, R.cochanges(ref["change"], a, b))), (a, b)
    ca, cb, co = engine.tree_cochanges(parent, tip_seq, [5], [5], 0)
    assert ca[0] == cb[0] == co[0] == ref["score"][5]
    three = np.array([4, 77, 128], dtype=np.int32)
    a, b = three[rng.integers(0, 3, size=1000)], three[rng.integers(0, 3, size=1000)]
    got = engine.tree_cochanges(parent, tip_seq, a, b, 0)
    assert all(np.array_equal(x, y) for x, y in zip(got, R.cochanges(ref["change"], a, b)))
    st = engine.tree_states(parent, tip_seq, [9, 100, 9], 0)
    assert np.array_equal(st[0], st[2]) and np.array_equal(st, ref["state"][[9, 100, 9]])


def test_the_context_keeps_its_alignment_and_weights(engine):
    rng = np.random.default_rng(13)
    states = R.random_alignment(rng, 130, 64)
    engine.set_alignment(states)
    thresh = 13
    before = (engine.get_alignment().tobytes(), engine.hamming_weights(thresh).tobytes())
    parent, tip_seq = R.balanced(list(range(64)))
    engine.tree_parsimony(parent, tip_seq, 0)
    engine.tree_states(parent, tip_seq, [1, 2], 1)
    engine.tree_cochanges(parent, tip_seq, [1, 2], [3, 4], 0)
    assert (engine.get_alignment().tobytes(), engine.hamming_weights(thresh).tobytes()) == before
    assert before[0] == states.tobytes()


def test_every_refusal_names_its_cause_and_leaves_the_context_working(engine):
    rng = np.random.default_rng(17)
    states = R.random_alignment(rng, 20, 9)
    parent, tip_seq = R.balanced(list(range(8)))          # 15 nodes; sequence 8 is in no tip
    nodes = len(parent)
    tips = np.flatnonzero(tip_seq >= 0)
    inner = np.flatnonzero(tip_seq < 0)
    with Engine(0) as fresh:                              # no alignment resident
        for call in (lambda: fresh.tree_parsimony(parent, tip_seq), lambda: fresh.tree_states(parent, tip_seq, [0]),
                     lambda: fresh.tree_cochanges(parent, tip_seq, [0], [0])):
            with pytest.raises(L.LdwError, match="no alignment resident") as e:
                call()
            assert e.value.code == L.LDW_ERR_STATE
    engine.set_alignment(states)
    ref = R.parsimony(parent, tip_seq, states, 0)

    def good():
        score, mn = engine.tree_parsimony(parent, tip_seq, 0)
        assert np.array_equal(score, ref["score"]) and np.array_equal(mn, ref["min_changes"])
        assert np.array_equal(engine.tree_states(parent, tip_seq, [19, 0], 0), ref["state"][[19, 0]])
        assert all(np.array_equal(x, y) for x, y in zip(engine.tree_cochanges(parent, tip_seq, [0, 4], [19, 4], 0), R.cochanges(ref["change"], [0, 4], [19, 4])))

    def changed(arr, at, value):
        out = arr.copy()
        out[at] = value
        return out

    bad_trees = [
        (parent[:1], tip_seq[:1], "1 nodes"),
        (np.array([-1, 0], dtype=np.int32), np.array([-1, 3], dtype=np.int32), "1 tips"),
        (changed(parent, 0, 0), tip_seq, r"parent\[0\] = 0"),
        (changed(parent, 5, 5), tip_seq, r"parent\[5\] = 5"),
        (changed(parent, 5, 9), tip_seq, r"parent\[5\] = 9"),
        (changed(parent, 7, -1), tip_seq, r"parent\[7\] = -1"),
        (parent, changed(tip_seq, tips[2], 9), f"tip node {tips[2]} names sequence 9"),
        (parent, changed(tip_seq, tips[2], -1), f"tip node {tips[2]} names sequence -1"),
        (parent, changed(tip_seq, tips[3], tip_seq[tips[1]]), f"tip nodes {tips[1]} and {tips[3]} both name sequence {tip_seq[tips[1]]}"),
        (parent, changed(tip_seq, inner[1], 8), f"node {inner[1]} has children but tip_seq 8"),
    ]
    for p, t, msg in bad_trees:
        for call in (lambda: engine.tree_parsimony(p, t, 0), lambda: engine.tree_states(p, t, [0], 0), lambda: engine.tree_cochanges(p, t, [0], [1], 0)):
            with pytest.raises(L.LdwError, match=msg) as e:
                call()
            assert e.value.code == L.LDW_ERR_ARG, msg
        good()
    bad_calls = [
        (lambda: engine.tree_parsimony(parent, tip_seq, 2), "gap_mode 2"),
        (lambda: engine.tree_states(parent, tip_seq, [0], -1), "gap_mode -1"),
        (lambda: engine.tree_cochanges(parent, tip_seq, [0], [0], 5), "gap_mode 5"),
        (lambda: engine.tree_states(parent, tip_seq, [0, 20], 0), r"snp_idx\[1\] = 20"),
        (lambda: engine.tree_states(parent, tip_seq, [-1], 0), r"snp_idx\[0\] = -1"),
        (lambda: engine.tree_cochanges(parent, tip_seq, [0, 1, 20], [0, 1, 2], 0), r"pair_a\[2\] = 20"),
        (lambda: engine.tree_cochanges(parent, tip_seq, [0, 1], [0, -3], 0), r"pair_b\[1\] = -3"),
        (lambda: engine.tree_states(parent, tip_seq, [], 0), "0 SNPs"),
        (lambda: engine.tree_cochanges(parent, tip_seq, [], [], 0), "0 pairs"),
    ]
    for call, msg in bad_calls:
        with pytest.raises(L.LdwError, match=msg) as e:
            call()
        assert e.value.code == L.LDW_ERR_ARG, msg
        good()
    lib, out = L.lib(), np.zeros(nodes * 2, dtype=np.int32)
    one = np.zeros(1, dtype=np.int32)
    args = (engine._ctx, L.ptr(parent), L.ptr(tip_seq), nodes, 0)
    assert lib.ldw_tree_parsimony(*args, None, L.ptr(out)) == L.LDW_ERR_ARG and b"output is null" in lib.ldw_last_error()
    assert lib.ldw_tree_parsimony(*args, L.ptr(out), None) == L.LDW_ERR_ARG
    assert lib.ldw_tree_states(*args, L.ptr(one), 1, None) == L.LDW_ERR_ARG and b"output is null" in lib.ldw_last_error()
    assert lib.ldw_tree_cochanges(*args, L.ptr(one), L.ptr(one), 1, L.ptr(out), None, L.ptr(out)) == L.LDW_ERR_ARG
    assert lib.ldw_tree_parsimony(engine._ctx, None, L.ptr(tip_seq), nodes, 0, L.ptr(out), L.ptr(out)) == L.LDW_ERR_ARG
    good()


def test_on_a_caller_owned_stream(engine):
    """The engine bound to a stream of the caller's (a torch stream that is not current) gives the own-stream engine's results, which are the
    reference's; the stream still works afterwards."""
    rng = np.random.default_rng(19)
    states = R.random_alignment(rng, 130, 65)
    parent, tip_seq = R.random_tree(rng, rng.permutation(65).tolist(), max_arity=5, p_unary=0.1)
    cs = J.CallerStream("not_current")
    try:
        with Engine(0, stream=cs.handle) as eng:
            eng.set_alignment(states)
            for gap_mode in (0, 1):
                check(eng, parent, tip_seq, states, gap_mode, rng, tag=("caller stream", gap_mode))
        assert cs.works()
    finally:
        cs.close()


def test_the_largest_case_1000_tips_5000_snps_on_the_nj_tree(engine):
    rng = np.random.default_rng(23)
    n, Ls = 1000, 5000
    states = R.random_alignment(rng, Ls, n)
    # (some structure for the tree to find: the second half of the sequences repeats the first at most columns)
    same = rng.random(Ls) < 0.7
    states[same, n // 2:] = states[same, :n // 2]
    engine.set_alignment(states)
    par, ln = engine.nj_tree()
    parent, tip_seq = R.from_tree(tree_from_joins(par, ln))
    sets, score = R.up_pass(parent, tip_seq, states, 0)
    got, mn = engine.tree_parsimony(parent, tip_seq, 0)
    assert np.array_equal(got, score) and np.array_equal(mn, R.min_changes(tip_seq, states, 0))
    a, b = some_pairs(rng, Ls, 250)
    cols = np.unique(np.concatenate([a, b]))
    _, change = R.down_pass(parent, np.ascontiguousarray(sets[:, cols]))
    ra, rb, rco = R.cochanges(np.ascontiguousarray(change.T), np.searchsorted(cols, a), np.searchsorted(cols, b))
    ca, cb, co = engine.tree_cochanges(parent, tip_seq, a, b, 0)
    assert np.array_equal(ca, ra) and np.array_equal(cb, rb) and np.array_equal(co, rco)
    assert np.array_equal(ca, score[a]) and np.array_equal(cb, score[b])


def test_python_surface_against_frames_built_from_the_reference(engine, tmp_path):
    import pandas as pd
    rng = np.random.default_rng(29)
    n, Ls = 40, 90
    states = R.random_alignment(rng, Ls, n)
    POS = (np.sort(rng.choice(np.arange(1, 5000), size=Ls, replace=False))).astype(np.int32)
    names = [f"iso{k}" for k in range(n)]
    snp = SnpDat.from_states(states, POS, 5000, seq_names=names)
    engine.set_alignment(states)
    par, ln = engine.nj_tree()
    tree = tree_from_joins(par, ln, labels=names)
    parent, tip_seq = R.from_tree(tree)
    assert np.array_equal(P.tip_sequences(tree, names), tip_seq)
    for gaps, gap_mode in (("missing", 0), ("state", 1)):
        ref = R.parsimony(parent, tip_seq, states, gap_mode)
        out = tmp_path / f"pars_{gaps}.tsv"
        df = P.snp_parsimony(tree, snp, engine=engine, gaps=gaps, out_path=out)
        assert list(df.columns) == ["POS", "score", "min_changes", "homoplasy", "ci"]
        assert np.array_equal(df["POS"], POS) and np.array_equal(df["score"], ref["score"]) and np.array_equal(df["min_changes"], ref["min_changes"])
        assert np.array_equal(df["homoplasy"], ref["score"] - ref["min_changes"])
        want_ci = np.where(ref["score"] == 0, 1.0, ref["min_changes"] / np.maximum(ref["score"], 1))
        assert np.array_equal(df["ci"], want_ci) and df["ci"][0] == 1.0
        back = pd.read_csv(out, sep="\t")
        assert np.array_equal(back["score"], ref["score"]) and list(back.columns) == list(df.columns)
        # links from a top-hits file
        a, b = some_pairs(rng, Ls, 25)
        links = pd.DataFrame({"pos1": POS[a], "pos2": POS[b], "len": np.abs(POS[a] - POS[b]), "MI": rng.random(25)})
        path = tmp_path / f"tophits_{gaps}.tsv"
        links.to_csv(path, sep="\t", index=False)
        got = P.link_cochanges(tree, str(path), snp, engine=engine, alignment_resident=True, gaps=gaps)
        ra, rb, rco = R.cochanges(ref["change"], a, b)
        assert list(got.columns) == ["pos1", "pos2", "len", "MI", "changes1", "changes2", "co_changes", "co_p"]
        assert np.array_equal(got["pos1"], POS[a]) and np.array_equal(got["pos2"], POS[b])
        assert np.array_equal(got["changes1"], ra) and np.array_equal(got["changes2"], rb) and np.array_equal(got["co_changes"], rco)
        want_p = [P.cochange_pvalue(tree.n_nodes - 1, int(x), int(y), int(z)) for x, y, z in zip(ra, rb, rco)]
        assert np.array_equal(got["co_p"], want_p)
        same = P.link_cochanges(tree, links, snp, engine=engine, gaps=gaps)
        # (MI went through text on its way into `got`: a frame's own columns come back as they were given)
        assert list(same.columns) == list(got.columns) and all(np.array_equal(same[c], got[c]) for c in got.columns if c != "MI")
        assert np.array_equal(same["MI"], links["MI"]) and list(links.columns) == ["pos1", "pos2", "len", "MI"]
        pos = [int(POS[3]), int(POS[80]), int(POS[3])]
        st = P.ancestral_states(tree, pos, snp, engine=engine, alignment_resident=True, gaps=gaps)
        assert st.dtype == np.uint8 and np.array_equal(st, ref["state"][[3, 80, 3]])
    with pytest.raises(ValueError, match="not a SNP position"):
        P.ancestral_states(tree, [int(POS.max()) + 1], snp, engine=engine, alignment_resident=True)
    with pytest.raises(ValueError, match="snp_dat.states is None"):
        P.snp_parsimony(tree, SnpDat(states=None, POS=POS, g=5000, uqe=None, r=None, seq_names=names), engine=engine)
