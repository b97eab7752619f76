"""Bootstrap support of the neighbour-joining tree on the device (ldw_nj_bootstrap) against its numpy statement (tests/nj_boot_ref.py over
tests/nj_ref.py): the reference tree and every replicate tree bit for bit, the support against exact tip sets, independence of the batch size, the
refusals, the context, and the Python layers up to the figure."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nj_boot_ref as BR                                    # noqa: E402
import nj_ref                                               # noqa: E402
import tree_ref as TR                                       # noqa: E402
from ldweaver_amd import _lib as L                         # noqa: E402
from ldweaver_amd import tree as T                         # noqa: E402

pytestmark = pytest.mark.gpu

MULT_CAP = 63       # csrc/ldw_nj.hip NJ_MULT_CAP: a biallelic column's digit 2 times 63 is the largest int8 digit the GEMM is given


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert got[1].dtype == np.float64 and np.array_equal(got[1], want[1])
    assert np.array_equal(np.signbit(got[1]), np.signbit(want[1]))


def _biallelic_column(st):
    return next(a for a in range(st.shape[0]) if len(np.unique(st[a])) == 2)


def _five_rows(st, seed):
    """B = 5: all ones; mostly zeros; random 0..63 with a biallelic column at 63; one column alone (a matrix of ties); a bootstrap draw."""
    Ls = st.shape[0]
    rng = np.random.default_rng(seed)
    a = _biallelic_column(st)
    sparse = np.where(rng.random(Ls) < 0.85, 0, rng.integers(1, 4, size=Ls))
    full = rng.integers(0, MULT_CAP + 1, size=Ls)
    full[a] = MULT_CAP
    one = np.zeros(Ls, dtype=np.int64)
    one[a] = 2
    return np.stack([np.ones(Ls, dtype=np.int64), sparse, full, one, T.bootstrap_multiplicities(Ls, 1, seed)[0]]).astype(np.int32)


def _check_against_the_reference(engine, st, mult):
    N = st.shape[1]
    engine.set_alignment(st)
    single = engine.nj_tree()
    parent, length, support, rp, rl = engine.nj_bootstrap(mult, want_trees=True)
    _same((parent, length), single)
    assert rp.shape == rl.shape == (len(mult), 2 * N - 2)
    for b, m in enumerate(mult):
        _same((rp[b], rl[b]), nj_ref.nj(BR.weighted_distance(st, m).astype(np.float64)))
    want = BR.support(parent, rp)
    assert support.dtype == np.int32 and np.array_equal(support, want)
    assert np.array_equal(engine.nj_bootstrap(mult)[2], want)      # without the replicates' trees kept
    return parent, support, rp


@pytest.mark.parametrize("N,Ls", [(3, 40), (4, 41), (5, 64), (65, 130), (129, 300), (257, 190)])
def test_replicate_trees_and_support_match_the_reference(engine, N, Ls):
    st = BR.five_state_alignment(Ls, N, seed=N)
    mult = _five_rows(st, seed=N)
    assert mult.max() == MULT_CAP and (mult[1] == 0).mean() > 0.6 and np.count_nonzero(mult[3]) == 1
    parent, support, rp = _check_against_the_reference(engine, st, mult)
    assert np.array_equal(rp[0], parent)                            # the row of ones is the alignment itself
    inner = support[N:2 * N - 3]
    assert len(inner) == N - 3 and (inner >= 1).all() and (inner <= 5).all()
    assert (support[:N] == -1).all() and support[2 * N - 3] == -1
    if N >= 65:
        assert (inner < 5).any()                                    # the replicates do disagree somewhere


def test_golden_alignment(engine, sample):
    st = np.ascontiguousarray(sample["states"])
    assert st.shape == (1268, 400)
    mult = T.bootstrap_multiplicities(1268, 3, seed=11)
    parent, support, _ = _check_against_the_reference(engine, st, mult)
    assert 0 < np.count_nonzero(support[400:797] == 3) < 397


def test_results_do_not_depend_on_the_batch(engine, tmp_path):
    st = BR.five_state_alignment(90, 70, seed=21)
    mult = np.concatenate([_five_rows(st, seed=21), T.bootstrap_multiplicities(90, 4, seed=5)])
    assert len(mult) == 9                                           # batches of 4, 4 and 1
    np.savez(tmp_path / "in.npz", states=st, mult=mult)
    env = dict(os.environ, LDW_NJ_BATCH="4")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "nj_boot_worker.py"), str(tmp_path / "in.npz"),
                        str(tmp_path / "out.npz")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.load(tmp_path / "out.npz")
    assert "LDW_NJ_BATCH" not in os.environ
    engine.set_alignment(st)
    here = dict(zip(("parent", "length", "support", "rep_parent", "rep_length"), engine.nj_bootstrap(mult, want_trees=True)))
    for name, a in here.items():
        for tag in ("b4", "b1", "default"):
            assert out[f"{tag}_{name}"].tobytes() == a.tobytes(), (tag, name)
    assert np.array_equal(here["support"], BR.support(here["parent"], here["rep_parent"]))


def _call(engine, mult, B, n, w):
    parent, length, support = np.empty(w, dtype=np.int32), np.empty(w, dtype=np.float64), np.empty(w, dtype=np.int32)
    return L.lib().ldw_nj_bootstrap(engine._ctx, L.ptr(mult), B, n, L.ptr(parent), L.ptr(length), L.ptr(support), None, None)


def test_refusals_leave_the_engine_usable(engine):
    from ldweaver_amd.engine import Engine
    st = BR.five_state_alignment(50, 20, seed=9)
    good = _five_rows(st, seed=9)
    engine.set_alignment(st)
    want = engine.nj_bootstrap(good, want_trees=True)
    too_many, negative = good.copy(), good.copy()
    too_many[2, 7] = MULT_CAP + 1
    negative[4, 0] = -1
    for bad in (too_many, negative):
        with pytest.raises(L.LdwError, match="multiplicity") as e:
            engine.nj_bootstrap(bad)
        assert e.value.code == L.LDW_ERR_ARG
    assert _call(engine, good, 5, 19, 38) == L.LDW_ERR_ARG           # n is not the alignment's N
    assert _call(engine, good, 0, 20, 38) == L.LDW_ERR_ARG           # no replicate
    assert _call(engine, None, 5, 20, 38) == L.LDW_ERR_ARG           # a null required pointer
    with pytest.raises(ValueError):
        engine.nj_bootstrap(good[:, :49])
    with Engine(0) as fresh:
        assert _call(fresh, good, 5, 20, 38) == L.LDW_ERR_STATE      # no alignment
        fresh.set_alignment(st)
        got = fresh.nj_bootstrap(good, want_trees=True)
    again = engine.nj_bootstrap(good, want_trees=True)
    for a, b, c in zip(want, got, again):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    _same(engine.nj_tree(), nj_ref.nj(BR.weighted_distance(st, np.ones(50)).astype(np.float64)))


def test_context_is_left_as_it_was(engine, sample):
    st = np.ascontiguousarray(sample["states"])
    engine.set_engine(L.ENGINE_MFMA)
    engine.set_alignment(st)
    thresh = int(st.shape[0] * 0.1)
    uqe = (engine.state_counts() > 0).T.astype(np.float64)
    hdw = engine.hamming_weights(thresh)
    engine.set_weights(hdw)
    engine.set_snp_meta(uqe.sum(axis=1), uqe, sample["POS"], np.ones(st.shape[0], dtype=np.int32), sample["g"])
    idx_f, idx_t = np.arange(0, 300), np.arange(200, 700)
    mi = engine.mi_block(idx_f, idx_t).copy()
    tree = engine.nj_tree()
    got = engine.nj_bootstrap(T.bootstrap_multiplicities(st.shape[0], 2, seed=3))
    _same(got[:2], tree)
    assert np.array_equal(engine.hamming_weights(thresh), hdw)
    assert np.array_equal(engine.mi_block(idx_f, idx_t), mi)
    assert np.array_equal(engine.get_alignment(), st)
    _same(engine.nj_tree(), tree)


def _split_support(tree):
    n = tree.n_nodes
    label_of = {int(v): tree.tip_label[t] for t, v in enumerate(tree.tip_node.tolist())}
    below = [frozenset([label_of[v]]) if v in label_of else frozenset() for v in range(n)]
    par = tree.parent.tolist()
    for v in range(n - 1, 0, -1):
        below[par[v]] = below[par[v]] | below[v]
    first, out = min(tree.tip_label), {}
    for v in range(1, n):
        if tree.support[v] >= 0:
            s = below[0] - below[v] if first in below[v] else below[v]
            assert out.setdefault(s, int(tree.support[v])) == int(tree.support[v])
    return out


def test_nj_tree_with_bootstrap(engine):
    N, Ls = 48, 120
    st = BR.five_state_alignment(Ls, N, seed=31)
    engine.set_alignment(st)
    tree = T.nj_tree(engine=engine, alignment_resident=True, bootstrap=4, seed=1)
    assert tree.n_replicates == 4 and tree.support.dtype == np.int32 and tree.support.shape == (2 * N - 2,)
    internal = np.diff(tree.child_ptr) > 0
    has = tree.support >= 0
    assert has.sum() == N - 3 and (tree.support[has] <= 4).all() and internal[has].all() and not has[0]
    assert (tree.support[~has] == -1).all()
    parent, _, support = engine.nj_bootstrap(T.bootstrap_multiplicities(Ls, 4, seed=1))
    want = {frozenset(str(t + 1) for t in s): int(support[u]) for s, u in BR.splits(parent).items()}
    want = {(frozenset(tree.tip_label) - s if "1" in s else s): v for s, v in want.items()}
    assert min(tree.tip_label) == "1" and _split_support(tree) == want
    back = T.parse_newick(T.write_newick(tree).encode())
    assert _split_support(back) == want
    rooted = T.ladderize(T.midpoint_root(back))
    assert _split_support(rooted) == want
    explicit = T.nj_tree(engine=engine, alignment_resident=True, multiplicities=T.bootstrap_multiplicities(Ls, 4, seed=1))
    assert np.array_equal(explicit.support, tree.support) and explicit.n_replicates == 4
    plain = T.nj_tree(engine=engine, alignment_resident=True)
    assert plain.support is None and np.array_equal(plain.parent, tree.parent) and np.array_equal(plain.length, tree.length)


def test_view_tree_marks_supported_nodes(engine, tmp_path):
    import pandas as pd
    N, Ls = 40, 80
    st = BR.five_state_alignment(Ls, N, seed=41)
    names = [f"iso{k:02d}" for k in range(N)]
    letters = np.frombuffer(b"ACGTN", dtype=np.uint8)[st.T]
    (tmp_path / "s.fa").write_bytes(b"".join(b">" + n.encode() + b"\n" + row.tobytes() + b"\n" for n, row in zip(names, letters)))
    (tmp_path / "s.pos").write_text("".join(f"{p}\n" for p in range(1, Ls + 1)))
    links = pd.DataFrame({"pos1": [2.0, 10.0], "pos2": [30.0, 55.0]})
    kw = dict(fasta_path=tmp_path / "s.fa", pos_file_path=tmp_path / "s.pos", links_df=links, plot_height=5, plot_width=5, dpi=30, engine=engine, want_canvas=True)
    out = T.view_tree(tree_path=None, bootstrap=4, seed=2, support_min=0.5, **kw)
    tree, lay, canvas = out["tree"], out["layout"], out["canvas"]
    assert tree.n_replicates == 4 and tree.support is not None
    internal = np.diff(tree.child_ptr) > 0
    marked = np.nonzero(internal & (tree.support >= 2))[0]
    assert len(marked) > 0 and np.array_equal(lay["support_nodes"], marked)
    plain = T.view_tree(tree_path=None, **kw)
    nb = len(plain["layout"]["bars"])
    assert plain["tree"].support is None and len(lay["bars"]) == nb + len(marked) and np.array_equal(lay["bars"][:nb], plain["layout"]["bars"])
    W, H = lay["canvas"]
    rows = [tuple(int(v) for v in b) for b in lay["bars"].tolist()]
    want = TR.paint_canvas(W, H, lay["panel"], rows, T.TREE_RGB, out["levels"], out["palette"], lay["bands"])
    for x, y, w, h in [lay["panel"]] + lay["bands"].tolist():
        assert np.array_equal(canvas[y:y + h, x:x + w], want[y:y + h, x:x + w])
    px, py, pw, ph = lay["panel"]
    assert not np.array_equal(canvas[py:py + ph, px:px + pw], plain["canvas"][py:py + ph, px:px + pw])
    # the same marks on the tree read from a file that carries the counts as internal labels
    nwk = tmp_path / "t.nwk"
    T.write_newick(_tree_of(st, names), nwk)
    ref = T.view_tree(tree_path=nwk, bootstrap=4, support_min=0.5, **kw)
    assert np.array_equal(ref["layout"]["bars"], lay["bars"]) and np.array_equal(ref["layout"]["support_nodes"], marked)
    assert len(T.view_tree(tree_path=nwk, **kw)["layout"]["support_nodes"]) == 0


def _tree_of(st, names):
    from ldweaver_amd.snpdat import SnpDat
    sd = SnpDat(states=st, POS=np.arange(st.shape[0], dtype=np.int32), g=None, uqe=None, r=None, seq_names=names)
    return T.nj_tree(sd, labels=names, bootstrap=4, seed=2)
