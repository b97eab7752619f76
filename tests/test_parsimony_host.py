"""Host: parsimony on a tree — the property the design rests on, checked on the numpy restatement; the host-side helpers of
ldweaver_amd/parsimony.py; what the three entry points refuse without a device."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import pars_ref as R
from ldweaver_amd import _lib as L
from ldweaver_amd import parsimony as P
from ldweaver_amd.tree import parse_newick

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("ldw_tree_parsimony", "ldw_tree_states", "ldw_tree_cochanges")


def test_score_down_pass_and_exact_minimum_agree_on_random_small_trees():
    """On 2 400 random trees — 2 to 14 tips, arity up to the tip count, unary nodes, about 20 % wildcard tips, both gap modes, three columns each — the up
    pass's score, the number of changes the down pass makes and the exact per-state dynamic programme are equal; every state lies in its node's set;
    under gap_mode 0 no branch to an N tip changes."""
    rng = np.random.default_rng(20240607)
    arities, unary = set(), 0
    for trial in range(2400):
        n = int(rng.integers(2, 15))
        gap_mode = trial & 1
        max_arity = int(rng.integers(2, n + 1))
        seqs = rng.permutation(n).tolist()
        parent, tip_seq = R.random_tree(rng, seqs, max_arity=max_arity, p_unary=0.15)
        states = R.random_alignment(rng, 3, n, p_n=0.2)
        if trial % 7 == 0:
            states[0] = 4                                  # an all-N column
        ar = np.bincount(parent[1:], minlength=len(parent))
        arities.update(ar.tolist())
        unary += int((ar == 1).any())
        sets, score = R.up_pass(parent, tip_seq, states, gap_mode)
        state, change = R.down_pass(parent, sets)
        exact = [R.sankoff_min(parent, tip_seq, states[c], gap_mode) for c in range(3)]
        assert score.tolist() == exact, (trial, parent.tolist(), states.tolist(), gap_mode)
        assert change.sum(axis=0).tolist() == exact, (trial, parent.tolist(), states.tolist(), gap_mode)
        assert np.all((sets >> state) & 1)
        assert not change[0].any()
        if gap_mode == 0:
            tips = np.flatnonzero(tip_seq >= 0)
            is_n = states[:, tip_seq[tips]].T == 4
            assert not (change[tips] & is_n).any()
        assert np.array_equal(R.min_changes(tip_seq, states, gap_mode) <= score, np.ones(3, dtype=bool))
    assert max(arities) >= 10 and 1 in arities and unary > 100      # the cases the statement names were drawn


def test_reference_on_a_tree_small_enough_to_follow_by_hand():
    """((A, A), (C, N)) under both gap modes, and a star of A, C, C, G."""
    parent, tip_seq = R.finish([-1, 0, 1, 1, 0, 4, 4], [0, 1, 2, 3])
    col = np.array([[0, 0, 1, 4]], dtype=np.uint8)
    r0, r1 = R.parsimony(parent, tip_seq, col, 0), R.parsimony(parent, tip_seq, col, 1)
    assert (r0["score"][0], r0["min_changes"][0]) == (1, 1) and (r1["score"][0], r1["min_changes"][0]) == (2, 2)
    assert r0["state"][0].tolist() == [0, 0, 0, 0, 1, 1, 1] and r0["change"][0].tolist() == [False] * 4 + [True, False, False]
    assert r1["state"][0].tolist() == [0, 0, 0, 0, 1, 1, 4]
    parent, tip_seq = R.star([0, 1, 2, 3])
    r = R.parsimony(parent, tip_seq, np.array([[0, 1, 1, 2]], dtype=np.uint8), 0)
    assert (r["score"][0], r["min_changes"][0]) == (2, 2) and r["state"][0].tolist() == [1, 0, 1, 1, 2]
    ca, cb, co = R.cochanges(r["change"], [0], [0])
    assert (ca[0], cb[0], co[0]) == (2, 2, 2)


def test_tree_shapes_of_the_reference_are_legal_trees():
    for make, n in ((R.caterpillar, 2), (R.caterpillar, 17), (R.balanced, 2), (R.balanced, 33), (R.star, 300)):
        parent, tip_seq = make(list(range(n)))
        assert parent[0] == -1 and np.all(parent[1:] < np.arange(1, len(parent))) and np.all(parent[1:] >= 0)
        assert sorted(tip_seq[tip_seq >= 0].tolist()) == list(range(n))
    parent, _ = R.caterpillar(list(range(17)))
    depth = np.zeros(len(parent), dtype=int)
    for v in range(1, len(parent)):
        depth[v] = depth[parent[v]] + 1
    assert depth.max() == 16


def test_tip_sequences_accepts_a_subset_in_any_order_and_rejects_bad_names():
    tree = parse_newick(b"((s3:1,s0:1):1,(s4:1,s1:1):1);")
    names = ["s0", "s1", "s2", "s3", "s4", "s5"]
    ts = P.tip_sequences(tree, names)
    assert ts.dtype == np.int32 and len(ts) == tree.n_nodes
    assert ts[tree.tip_node].tolist() == [3, 0, 4, 1] and np.all(ts[np.setdiff1d(np.arange(tree.n_nodes), tree.tip_node)] == -1)
    with pytest.raises(ValueError, match="Sequence names mismatch between provided tree file and fasta file"):
        P.tip_sequences(tree, ["s0", "s1", "s3"])                       # s4 is missing
    with pytest.raises(ValueError, match="Sequence names mismatch between provided tree file and fasta file"):
        P.tip_sequences(tree, names + ["s3"])                           # s3 is held twice
    assert P.tip_sequences(tree, names + ["s5"]).tolist() == ts.tolist()    # a name no tip uses may repeat


def exact_tail(M, n1, n2, co):
    tot = Fraction(0)
    for x in range(max(co, 0), min(n1, n2) + 1):
        if n2 - x <= M - n1:
            tot += Fraction(math.comb(n1, x) * math.comb(M - n1, n2 - x), math.comb(M, n2))
    return tot


def test_cochange_pvalue_equals_the_exact_sum():
    """Against sums of exact fractions.  The tolerance is the lgamma route's own: a term is exp of nine lgamma values of size at most lgamma(M + 1),
    each good to a few ulp, so its relative error is about 9 x 4 x 2^-52 x lgamma(M + 1): 1e-12 at M = 40 (lgamma 110), 1e-10 at M = 1999
    (lgamma 13 200); ten times that is allowed."""
    for M in (1, 2, 5, 12, 40):
        for n1 in range(M + 1):
            for n2 in range(M + 1):
                for co in range(-1, min(n1, n2) + 3):
                    got, want = P.cochange_pvalue(M, n1, n2, co), float(exact_tail(M, n1, n2, co))
                    assert abs(got - want) <= 1e-11 * want, (M, n1, n2, co, got, want)
    assert P.cochange_pvalue(1999, 30, 40, 0) == 1.0
    assert P.cochange_pvalue(1999, 30, 40, 31) == 0.0
    p = [P.cochange_pvalue(1999, 30, 40, c) for c in range(0, 31)]
    assert all(a >= b for a, b in zip(p, p[1:])) and 0.0 < p[30] < 1e-40
    for c in (1, 5, 30):
        assert abs(p[c] - float(exact_tail(1999, 30, 40, c))) <= 1e-9 * p[c]
    with pytest.raises(ValueError):
        P.cochange_pvalue(10, 11, 2, 1)


def test_python_surface_refuses_bad_arguments_before_it_needs_a_device():
    tree = parse_newick(b"(a:1,b:1,c:1);")
    with pytest.raises(ValueError, match="gaps must be one of"):
        P.snp_parsimony(tree, None, gaps="ignore")
    with pytest.raises(ValueError, match="alignment_resident=True needs the engine"):
        P.snp_parsimony(tree, None, alignment_resident=True)
    with pytest.raises(ValueError, match="no alignment"):
        P.snp_parsimony(tree, None)
    with pytest.raises(ValueError, match="positions need snp_dat.POS"):
        P.ancestral_states(tree, [1, 2], None)
    import ldweaver_amd
    for name in ("snp_parsimony", "link_cochanges", "ancestral_states", "tip_sequences", "cochange_pvalue"):
        assert getattr(ldweaver_amd, name) is getattr(P, name)


def test_entry_points_are_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldweaver_amd.h")).read(), flags=re.S)
    lib = L.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in L.declared_symbols() and hasattr(lib, name)


def test_entry_points_refuse_a_null_context_without_a_gpu():
    """In the style of test_new_entry_points_refuse_bad_arguments_without_a_gpu: without a context nothing else can be examined, and the answer is
    LDW_ERR_ARG with a message, never a crash."""
    lib = L.lib()
    parent, tip_seq = R.star([0, 1, 2])
    out = np.zeros(8, dtype=np.int32)
    idx = np.zeros(1, dtype=np.int32)
    st = np.zeros(4, dtype=np.uint8)
    assert lib.ldw_tree_parsimony(None, L.ptr(parent), L.ptr(tip_seq), 4, 0, L.ptr(out), L.ptr(out)) == L.LDW_ERR_ARG
    assert b"null context" in lib.ldw_last_error()
    assert lib.ldw_tree_states(None, L.ptr(parent), L.ptr(tip_seq), 4, 0, L.ptr(idx), 1, L.ptr(st)) == L.LDW_ERR_ARG
    assert b"null context" in lib.ldw_last_error()
    assert lib.ldw_tree_cochanges(None, L.ptr(parent), L.ptr(tip_seq), 4, 0, L.ptr(idx), L.ptr(idx), 1, L.ptr(out), L.ptr(out), L.ptr(out)) == L.LDW_ERR_ARG
    assert b"null context" in lib.ldw_last_error()
    assert lib.ldw_tree_parsimony(None, None, None, 0, 7, None, None) == L.LDW_ERR_ARG
