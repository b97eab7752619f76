"""The neighbour-joining tree on the device (ldw_nj_tree) against the numpy statement of the algorithm (tests/nj_ref.py): bit for bit
on matrices full of ties, on the resident alignment, across buffer reuse; the refusals; view_tree without a tree file."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nj_ref                                               # noqa: E402
from ldweaver_amd import _lib as L                         # noqa: E402
from ldweaver_amd import tree as T                         # noqa: E402
from ldweaver_amd.snpdat import SnpDat                     # noqa: E402

pytestmark = pytest.mark.gpu

NJ_THREADS = 256        # csrc/ldw_nj.hip: threads of a workgroup = the columns a scan's workgroup takes per step
NJ_MAX_PARTIALS = 512   # csrc/ldw_nj.hip: most workgroups of a scan = entries of the partial-minimum array; beyond it a workgroup takes several rows
NJ_UNROLL = 4           # csrc/ldw_nj.hip: column tiles a scan's workgroup takes per step: past NJ_UNROLL * NJ_THREADS columns a thread takes a second step
SIZES = [3, 4, 5, 63, 64, 65, 129, NJ_THREADS - 1, NJ_THREADS, NJ_THREADS + 1, 400, NJ_MAX_PARTIALS - 1, NJ_MAX_PARTIALS, NJ_MAX_PARTIALS + 1]
assert 257 in SIZES


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert got[1].dtype == np.float64 and np.array_equal(got[1], want[1])
    assert np.array_equal(np.signbit(got[1]), np.signbit(want[1]))


@pytest.mark.parametrize("N", SIZES)
def test_matrix_route_matches_the_reference(engine, N):
    mats = {"ties": nj_ref.tie_matrix(N, seed=N), "zero": np.zeros((N, N)), "additive": nj_ref.random_tree_matrix(N, seed=N),
            "largest ids first": nj_ref.last_first_matrix(N)}
    if N >= 6:
        mats["a in the last slot"] = nj_ref.last_slot_a_matrix(N)
    for name, d in mats.items():
        want = nj_ref.nj(d)
        got = engine.nj_tree(d)
        assert got[0][2 * N - 3] == -1 and got[1][2 * N - 3] == 0.0, name
        assert np.array_equal(got[0], want[0]), name
        assert np.array_equal(got[1], want[1]), name
        _same(got, want)
    if N >= 6:
        p = engine.nj_tree(mats["largest ids first"])[0]
        assert p[N - 1] == p[N - 2] == N and p[N - 3] == p[N] == N + 1
        p = engine.nj_tree(mats["a in the last slot"])[0]
        assert p[0] == p[1] == N and p[N - 2] == p[N] == N + 1
    if N >= 65:
        assert (engine.nj_tree(mats["ties"])[1] < 0).any()


def test_scan_takes_a_second_step(engine):
    N = NJ_UNROLL * NJ_THREADS + 1
    d = nj_ref.tie_matrix(N, seed=N)
    _same(engine.nj_tree(d), nj_ref.nj(d))


def test_zero_matrix_is_the_id_rule(engine):
    parent, length = engine.nj_tree(np.zeros((33, 33)))
    assert parent[:8].tolist() == [33, 33, 34, 34, 35, 35, 36, 36] and not length.any()


def test_additive_matrix_beyond_the_reference(engine):
    N = 1500
    d = nj_ref.random_tree_matrix(N, seed=11)
    parent, length = engine.nj_tree(d)
    assert parent[2 * N - 3] == -1 and np.all(parent[:2 * N - 3] >= N) and np.all(parent[:2 * N - 3] <= 2 * N - 3)
    assert np.array_equal(np.bincount(parent[:2 * N - 3], minlength=2 * N - 2)[N:], [2] * (N - 3) + [3])
    tips = np.random.default_rng(2).choice(N, 16, replace=False)
    assert np.array_equal(nj_ref.patristic(parent, length, tips.tolist()), d[tips])


@pytest.fixture(scope="module")
def golden_states(sample):
    st = np.ascontiguousarray(sample["states"])
    assert st.shape == (1268, 400)
    return st


def test_alignment_route(engine, golden_states):
    st = golden_states
    Ls = st.shape[0]
    engine.set_alignment(st)
    from_alignment = engine.nj_tree()
    _, shared = engine.hamming_weights(int(Ls * 0.1), want_shared=True)
    d = (Ls - shared).astype(np.float64)
    assert int(((d == 0).sum() - 400) // 2) == 878      # identical sequence pairs: ties are plentiful
    _same(from_alignment, engine.nj_tree(d))
    _same(from_alignment, nj_ref.nj(d))
    tree = T.nj_tree(engine=engine, alignment_resident=True, labels=[f"s{k}" for k in range(400)], per_site=True, clamp_negative=False)
    raw = T.tree_from_joins(*from_alignment, clamp_negative=False)
    assert np.array_equal(tree.parent, raw.parent) and np.array_equal(tree.length, raw.length / Ls) and tree.tip_label[3] == "s3"
    sd = SnpDat.from_states(st, sample_pos(st), None, seq_names=[f"n{k}" for k in range(400)])
    tree = T.nj_tree(sd, engine=engine)
    assert tree.tip_label == sd.seq_names and tree.length.min() >= 0 and T.midpoint_root(tree).n_tips == 400


def sample_pos(st):
    return np.arange(1, st.shape[0] + 1, dtype=np.int32)


def test_context_is_left_as_it_was(engine, sample, golden_states):
    st = golden_states
    engine.set_engine(L.ENGINE_MFMA)
    engine.set_alignment(st)
    thresh = int(st.shape[0] * 0.1)
    uqe = (engine.state_counts() > 0).T.astype(np.float64)
    hdw = engine.hamming_weights(thresh)
    engine.set_weights(hdw)
    engine.set_snp_meta(uqe.sum(axis=1), uqe, sample["POS"], np.ones(st.shape[0], dtype=np.int32), sample["g"])
    idx_f, idx_t = np.arange(0, 300), np.arange(200, 700)
    mi = engine.mi_block(idx_f, idx_t).copy()
    engine.nj_tree()
    engine.nj_tree(nj_ref.tie_matrix(70, seed=3))
    assert np.array_equal(engine.hamming_weights(thresh), hdw)
    assert np.array_equal(engine.mi_block(idx_f, idx_t), mi)
    assert np.array_equal(engine.get_alignment(), st)


def test_buffers_reused_larger_smaller_larger():
    from ldweaver_amd.engine import Engine
    mats = [nj_ref.tie_matrix(257, seed=5), nj_ref.tie_matrix(64, seed=6), nj_ref.tie_matrix(257, seed=7)]
    with Engine(0) as one:
        got = [one.nj_tree(d) for d in mats]
    for d, g in zip(mats, got):
        with Engine(0) as fresh:
            _same(g, fresh.nj_tree(d))
        _same(g, nj_ref.nj(d))


def test_refusals_leave_the_engine_usable(engine):
    good = nj_ref.tie_matrix(20, seed=1)
    want = nj_ref.nj(good)
    asym = good.copy()
    asym[3, 7] += 1.0
    diag = good.copy()
    diag[5, 5] = 1.0
    nan = good.copy()
    nan[2, 9] = nan[9, 2] = np.nan
    inf = good.copy()
    inf[2, 9] = inf[9, 2] = np.inf
    for bad, word in ((asym, "symmetric"), (diag, "diagonal"), (nan, "finite"), (inf, "finite")):
        with pytest.raises(L.LdwError, match=word) as e:
            engine.nj_tree(bad)
        assert e.value.code == L.LDW_ERR_ARG
        _same(engine.nj_tree(good), want)
    with pytest.raises(L.LdwError) as e:
        engine.nj_tree(np.zeros((2, 2)))
    assert e.value.code == L.LDW_ERR_ARG
    with pytest.raises(ValueError):
        engine.nj_tree(np.zeros((4, 5)))
    _same(engine.nj_tree(good), want)


def test_no_alignment_no_tree():
    from ldweaver_amd.engine import Engine
    with Engine(0) as eng:
        with pytest.raises(L.LdwError) as e:
            eng.nj_tree()
        assert e.value.code == L.LDW_ERR_STATE
        eng.set_alignment(np.zeros((10, 5), dtype=np.uint8))
        parent, length = eng.nj_tree()
        assert parent.tolist() == [5, 5, 6, 6, 7, 7, 7, -1] and not length.any()
    with pytest.raises(ValueError):
        T.nj_tree()


def test_view_tree_builds_its_own_tree(engine, sample, golden_states, tmp_path):
    import pandas as pd
    st = golden_states
    names = [f"iso{k:03d}" for k in range(400)]
    letters = np.frombuffer(b"ACGTN", dtype=np.uint8)[st.T]
    (tmp_path / "s.fa").write_bytes(b"".join(b">" + n.encode() + b"\n" + row.tobytes() + b"\n" for n, row in zip(names, letters)))
    pos = sample["POS"].astype(np.int64)
    (tmp_path / "s.pos").write_text("".join(f"{p}\n" for p in pos.tolist()))
    links = pd.DataFrame({"pos1": pos[[3, 40, 500]].astype(float), "pos2": pos[[90, 700, 1200]].astype(float)})
    kw = dict(fasta_path=tmp_path / "s.fa", pos_file_path=tmp_path / "s.pos", links_df=links, plot_height=4, plot_width=5, dpi=100, engine=engine,
              want_canvas=True)
    out = T.view_tree(tree_path=None, **kw)
    assert out["tree"].n_tips == 400 and sorted(out["tree"].tip_label) == names
    assert len(out["pos_plot"]) == 6
    sd = SnpDat.from_states(st, np.arange(st.shape[0]), None, seq_names=names)
    nwk = tmp_path / "NJ (Hamming)"       # the figure's title is the file's name: the one the built tree gets
    T.write_newick(T.nj_tree(sd, engine=engine), nwk)
    ref = T.view_tree(tree_path=nwk, **kw)
    assert out["canvas"].shape == (400, 500, 3) and out["canvas"].tobytes() == ref["canvas"].tobytes()
    assert np.array_equal(out["boxes"], ref["boxes"]) and np.any(out["canvas"] != 255)
    assert np.array_equal(out["tree"].parent, ref["tree"].parent) and np.array_equal(out["tree"].length, ref["tree"].length)
