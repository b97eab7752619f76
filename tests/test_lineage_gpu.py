"""GPU: the lineage check (ldw_seq_clusters, ldw_links_stratified) against the numpy restatement tests/lineage_ref.py and the oracle
(pytest -m gpu).  Integers are compared with array_equal, MI within MI_TIGHT."""
import math

import numpy as np
import pytest

import caller_stream_job as J
import ldw_oracle as orc
import lineage_ref as R
from ldweaver_amd import _lib as L
from ldweaver_amd import lineage as G
from ldweaver_amd.engine import Engine
from ldweaver_amd.snpdat import SnpDat
from ldweaver_amd.synth import synth_alignment

pytestmark = pytest.mark.gpu

MI_TIGHT = 1e-10       # what the 40-bit fixed-point weights deliver
L_CLU, T_CLU = 257, 20


# ---- clusters -------------------------------------------------------------------------------------------------------------------------------------
def change(rng, seq, n):
    """``seq`` with exactly n columns changed (returns the copy and the columns)."""
    cols = rng.choice(len(seq), n, replace=False)
    out = seq.copy()
    out[cols] = (out[cols] + rng.integers(1, 4, n)) % 4
    return out, cols


def founders_alignment(rng, N, Ls=L_CLU, t=T_CLU):
    """(states (Ls, N), joined pair, split pair): a few far-apart founders with members 0 to 3 mutations away (bimodal distances); q1 and p1 alone at
    distance exactly t - 1 (joined), q2 and p2 alone at exactly t (not joined).  q1 sits at sequence 1, p1 at the LAST sequence: from 129 sequences on the
    only edge of their cluster joins a sequence below 128 to one at or above it, where G has its 128-sequence tiles.  With 2 or 3 sequences: q1, p1, and
    a third at distance t from q1 and 2 t - 1 from p1."""
    q1 = rng.integers(0, 4, Ls).astype(np.uint8)
    p1, cols = change(rng, q1, t - 1)
    if N <= 3:
        rest = np.setdiff1d(np.arange(Ls), cols)
        p2 = q1.copy()
        c2 = rng.choice(rest, t, replace=False)
        p2[c2] = (p2[c2] + 1) % 4
        seqs = [q1, p1, p2][:N]
        return np.stack(seqs, axis=1), (0, 1), ((0, 2) if N == 3 else None)
    q2 = rng.integers(0, 4, Ls).astype(np.uint8)
    p2, _ = change(rng, q2, t)
    seqs = [q2, q1, p2]
    n_f = max(1, min(5, (N - 4) // 3))
    founders = [rng.integers(0, 5, Ls).astype(np.uint8) for _ in range(n_f)]
    while len(seqs) < N - 1:
        seqs.append(change(rng, founders[int(rng.integers(n_f))], int(rng.integers(0, 4)))[0] if founders else q2)
    seqs.append(p1)
    return np.stack(seqs, axis=1), (1, N - 1), (0, 2)


def check_partition(lab, n, ref_lab, ref_n, tag):
    assert int(n) == int(ref_n) and np.array_equal(lab, ref_lab), (tag, int(n), int(ref_n))


@pytest.mark.parametrize("N", (2, 3, 64, 65, 127, 128, 129, 257, 300))
def test_clusters_of_founders_and_mutants_with_pairs_at_the_threshold(engine, N):
    rng = np.random.default_rng(N)
    st, joined, split = founders_alignment(rng, N)
    engine.set_alignment(st)
    ref_lab, ref_n = R.seq_clusters(st, [T_CLU])
    lab, n = engine.seq_clusters(T_CLU)
    assert lab.dtype == np.int32 and lab.shape == (N,)
    check_partition(lab, n, ref_lab[0], ref_n[0], N)
    d = lambda i, j: int((st[:, i] != st[:, j]).sum())
    assert d(*joined) == T_CLU - 1 and lab[joined[0]] == lab[joined[1]]
    assert (lab == lab[joined[0]]).sum() == 2                       # the one edge of that cluster
    if split:
        assert d(*split) == T_CLU and lab[split[0]] != lab[split[1]]
    t = engine.last_timing()
    assert 1 <= t["select_ms"] <= 4 * max(1, math.ceil(math.log2(N))) and t["total_ms"] > 0 and abs(t["gemm_ms"] + t["epilogue_ms"] - t["total_ms"]) < 1e-3


@pytest.mark.parametrize("N", (3, 65, 129, 300))
def test_the_thresholds_zero_one_and_past_the_alignment(engine, N):
    rng = np.random.default_rng(100 + N)
    st, _, _ = founders_alignment(rng, N)
    st[:, -1] = st[:, 0]                                          # two identical sequences, first and last
    engine.set_alignment(st)
    lab, n = engine.seq_clusters([0, 1, L_CLU + 1])
    ref_lab, ref_n = R.seq_clusters(st, [0, 1, L_CLU + 1])
    assert np.array_equal(lab, ref_lab) and np.array_equal(n, ref_n)
    assert np.array_equal(lab[0], np.arange(N)) and n[0] == N     # no sequence is even its own neighbour
    assert lab[1][0] == lab[1][-1] == 0 and n[1] < N                # identical sequences join
    assert not lab[2].any() and n[2] == 1


@pytest.mark.parametrize("N", (65, 129, 300))
def test_three_thresholds_in_one_call_are_three_calls_nested_and_bound_the_neighbour_counts(engine, N):
    rng = np.random.default_rng(200 + N)
    st, _, _ = founders_alignment(rng, N)
    engine.set_alignment(st)
    th = [3, T_CLU, 150]
    lab, n = engine.seq_clusters(th)
    ref_lab, ref_n = R.seq_clusters(st, th)
    assert np.array_equal(lab, ref_lab) and np.array_equal(n, ref_n)
    for k, t in enumerate(th):
        one, n_one = engine.seq_clusters(t)
        assert np.array_equal(one, lab[k]) and n_one == n[k], t
        hdw = engine.hamming_weights(t)
        size = np.bincount(lab[k])[lab[k]]
        assert np.all(np.rint(1.0 / hdw - 1.0) <= size), t        # a sequence's neighbours (itself among them) lie in its cluster
    assert n[0] > n[1] >= n[2]
    for k in (0, 1):                                               # a larger t only merges: a finer cluster lies in one coarser cluster
        coarse_of = {}
        for fine, coarse in zip(lab[k].tolist(), lab[k + 1].tolist()):
            assert coarse_of.setdefault(fine, coarse) == coarse


def chain(N):
    """(N - 1, N): sequence k has the first k columns flipped, so d(i, j) = |i - j|."""
    return (np.arange(N - 1)[:, None] < np.arange(N)[None, :]).astype(np.uint8)


@pytest.mark.parametrize("numbering", ("sorted", "reversed", "shuffled"))
def test_a_chain_of_1024_sequences_is_one_cluster_in_few_rounds(engine, numbering):
    """Single linkage makes chains, and minimum-label propagation takes N - 1 rounds on one: the cap of 4 ceil(log2 N) rounds rules it out."""
    N = 1024
    rng = np.random.default_rng(5)
    order = dict(sorted=np.arange(N), reversed=np.arange(N)[::-1], shuffled=rng.permutation(N))[numbering]
    st = np.ascontiguousarray(chain(N)[:, order])
    engine.set_alignment(st)
    lab, n = engine.seq_clusters(2)
    assert n == 1 and not lab.any()
    rounds = engine.last_timing()["select_ms"]
    print(f"chain of {N}, {numbering}: {rounds:.0f} rounds")
    assert 1 <= rounds <= 4 * math.ceil(math.log2(N))
    # without two sequences in the middle the chain is two
    keep = order[(order != 511) & (order != 512)]
    st2 = np.ascontiguousarray(chain(N)[:, keep])
    engine.set_alignment(st2)
    lab2, n2 = engine.seq_clusters(2)
    ref_lab, ref_n = R.seq_clusters(st2, [2])
    assert n2 == 2 == ref_n[0] and np.array_equal(lab2, ref_lab[0]) and sorted(np.bincount(lab2).tolist()) == [511, 511]
    assert engine.last_timing()["select_ms"] <= 4 * math.ceil(math.log2(N))


def test_clusters_on_a_caller_owned_stream():
    rng = np.random.default_rng(31)
    st, _, _ = founders_alignment(rng, 129)
    ref_lab, ref_n = R.seq_clusters(st, [T_CLU, 150])
    cs = J.CallerStream("not_current")
    try:
        with Engine(0, stream=cs.handle) as eng:
            eng.set_alignment(st)
            lab, n = eng.seq_clusters([T_CLU, 150])
            assert np.array_equal(lab, ref_lab) and np.array_equal(n, ref_n)
            hdw = eng.hamming_weights(T_CLU)
            eng.set_weights(hdw)
            a, b = some_pairs(rng, L_CLU, 12)
            res = eng.links_stratified(a, b, lab[0], int(n[0]), want_tables=True)
            check_stratified(res, R.links_stratified(st, hdw, a, b, lab[0], int(n[0])), "caller stream")
        assert cs.works()
    finally:
        cs.close()


def test_clusters_refusals_leave_the_context_usable():
    lib = L.lib()
    with Engine(0) as eng:
        with pytest.raises(L.LdwError) as e:
            eng.seq_clusters(3)
        assert e.value.code == L.LDW_ERR_STATE
        st, _, _ = founders_alignment(np.random.default_rng(1), 65)
        eng.set_alignment(st)
        for bad in ([], list(range(17)), [3, -1]):
            with pytest.raises(L.LdwError) as e:
                eng.seq_clusters(bad)
            assert e.value.code == L.LDW_ERR_ARG, bad
        th, lab, n = np.array([3], dtype=np.int32), np.zeros(65, dtype=np.int32), np.zeros(1, dtype=np.int32)
        for args in ((None, 1, L.ptr(lab), L.ptr(n)), (L.ptr(th), 1, None, L.ptr(n)), (L.ptr(th), 1, L.ptr(lab), None)):
            assert lib.ldw_seq_clusters(eng._ctx, *args) == L.LDW_ERR_ARG
        lab, n = eng.seq_clusters(T_CLU)
        ref_lab, ref_n = R.seq_clusters(st, [T_CLU])
        assert np.array_equal(lab, ref_lab[0]) and n == ref_n[0]
        assert np.array_equal(eng.get_alignment(), st)


# ---- stratified tables and MI -----------------------------------------------------------------------------------------------------------------------
def some_pairs(rng, Ls, K):
    """K pairs among Ls SNPs; where K allows, the first is a == b and the last two are one pair twice."""
    a, b = rng.integers(0, Ls, size=K).astype(np.int32), rng.integers(0, Ls, size=K).astype(np.int32)
    b[0] = a[0]
    if K >= 3:
        a[-1], b[-1] = a[-2], b[-2]
    return a, b


def random_states(rng, Ls, N):
    """Clonal groups of 1, 2, 3 and 5 sequences in turn, so that the Hamming weights have a few classes."""
    gid = np.repeat(np.arange(N), np.resize([1, 2, 3, 5], N))[:N]
    st = rng.choice(5, size=(Ls, N), p=[0.45, 0.3, 0.15, 0.07, 0.03]).astype(np.uint8)[:, gid]
    st[0] = 1                                                       # a monomorphic SNP
    if Ls > 2:
        st[2] = rng.integers(0, 2, N)                               # a biallelic one
    return st


def some_labels(rng, N, Cn):
    """Labels in [-1, Cn): where the sizes allow, one sequence left out, a cluster of one, a cluster id without a member, and — the others drawn with
    uneven odds — clusters that begin and end inside one 64-bit word of the sorted order."""
    if Cn == N:
        return rng.permutation(N).astype(np.int32)
    ids = np.arange(Cn)
    empty = Cn - 1 if Cn >= 3 else -2
    single = 0 if Cn >= 3 and N > 4 else -2
    pool = ids[(ids != empty) & (ids != single)]
    w = 1.0 / (1.0 + np.arange(len(pool)))
    lab = rng.choice(pool, size=N, p=w / w.sum()).astype(np.int32)
    if single >= 0:
        lab[int(rng.integers(N))] = single
    if N > 2:
        free = np.nonzero(lab != single)[0]
        lab[free[int(rng.integers(len(free)))]] = -1
    return lab


def weights_of(kind, rng, engine, st):
    N = st.shape[1]
    if kind == "hamming":
        return engine.hamming_weights(int(st.shape[0] * 0.3))
    if kind == "distinct":
        return (1.0 + rng.permutation(N)) / (N + 1.0)               # every weight its own class: one piece per sequence
    return np.ones(N)


def check_stratified(res, ref, tag):
    assert res["frac_bits"] == ref["frac_bits"], tag
    assert np.array_equal(res["counts"], ref["counts"]) and np.array_equal(res["fixed"], ref["fixed"]), tag
    assert np.array_equal(res["poly"], ref["poly"]) and np.array_equal(res["neff"], ref["neff"]), tag
    assert np.isfinite(res["mi"]).all() and np.abs(res["mi"] - ref["mi"]).max() < MI_TIGHT, (tag, np.abs(res["mi"] - ref["mi"]).max())
    assert np.abs(res["mi_all"] - ref["mi_all"]).max() < MI_TIGHT, tag
    assert not res["mi"][res["poly"] == 0].any(), tag              # exactly 0 where both SNPs are monomorphic in the cluster


@pytest.mark.parametrize("kind", ("hamming", "distinct", "unit"))
@pytest.mark.parametrize("N", (2, 63, 64, 65, 128, 129, 200))
def test_tables_and_mi_per_cluster_against_the_reference_and_the_oracle(engine, N, kind):
    rng = np.random.default_rng(1000 * N + len(kind))
    Ls = 40
    st = random_states(rng, Ls, N)
    engine.set_alignment(st)
    hdw = weights_of(kind, rng, engine, st)
    engine.set_weights(hdw)
    for Cn in (1, 2, 3, 64, 65) + ((N,) if N == 65 else ()):
        lab = some_labels(rng, N, Cn)
        for K in (1, 9):
            a, b = some_pairs(rng, Ls, K)
            res = engine.links_stratified(a, b, lab, Cn, want_tables=True)
            ref = R.links_stratified(st, hdw, a, b, lab, Cn)
            check_stratified(res, ref, (N, kind, Cn, K))
            if kind == "unit":
                assert res["frac_bits"] == 0 and np.array_equal(res["fixed"], res["counts"])
            lean = engine.links_stratified(a, b, lab, Cn)             # without the tables: the same bits
            assert set(lean) == {"mi", "mi_all", "poly", "neff", "frac_bits"}
            assert lean["mi"].tobytes() == res["mi"].tobytes() and lean["mi_all"].tobytes() == res["mi_all"].tobytes()
        # the oracle itself on the members of two clusters, for the last pairs
        for c in np.unique(lab[lab >= 0])[:2].tolist():
            mem = lab == c
            uqe, r = orc.uqe_r(st[:, mem])
            for k in range(min(K, 3)):
                want = orc.mi_pair_direct(st[:, mem], hdw[mem], r, uqe, int(a[k]), int(b[k]))
                assert abs(res["mi"][k, c] - want) < MI_TIGHT, (N, kind, Cn, c, k)


@pytest.mark.parametrize("kind", ("hamming", "distinct", "unit"))
def test_every_sequence_labelled_sums_to_the_joint_tables_and_the_dense_mi(engine, kind):
    rng = np.random.default_rng(77 + len(kind))
    Ls, N, Cn = 60, 129, 7
    st = random_states(rng, Ls, N)
    engine.set_alignment(st)
    hdw = weights_of(kind, rng, engine, st)
    engine.set_weights(hdw)
    lab = rng.integers(0, Cn, N).astype(np.int32)
    a, b = some_pairs(rng, Ls, 25)
    res = engine.links_stratified(a, b, lab, Cn, want_tables=True)       # (before the SNP meta data are there: it does not need them)
    uqe, r = orc.uqe_r(st)
    engine.set_snp_meta(r, uqe, np.arange(1, Ls + 1, dtype=np.int32), None, float(Ls + 1))
    cnt, fix, fb = engine.joint_tables(a, b)
    assert fb == res["frac_bits"] and np.array_equal(res["counts"].sum(axis=1), cnt) and np.array_equal(res["fixed"].sum(axis=1), fix)
    dense = engine.mi_block(np.arange(Ls), np.arange(Ls), quirk=L.QUIRK_INTENDED)
    assert np.abs(res["mi_all"] - dense[a, b]).max() < MI_TIGHT
    assert abs(res["neff"].sum() - float(np.sum(hdw.astype(np.longdouble)))) < 1e-9


def test_forty_pairs_in_chunks_of_seven_and_permuted_cluster_ids_give_the_same_bits(engine, monkeypatch):
    rng = np.random.default_rng(40)
    Ls, N, Cn = 50, 200, 9
    st = random_states(rng, Ls, N)
    engine.set_alignment(st)
    hdw = engine.hamming_weights(15)
    engine.set_weights(hdw)
    lab = some_labels(rng, N, Cn)
    a, b = some_pairs(rng, Ls, 40)
    monkeypatch.delenv("LDW_LIN_CHUNK", raising=False)
    want = engine.links_stratified(a, b, lab, Cn, want_tables=True)
    check_stratified(want, R.links_stratified(st, hdw, a, b, lab, Cn), "default chunk")
    monkeypatch.setenv("LDW_LIN_CHUNK", "7")
    got = engine.links_stratified(a, b, lab, Cn, want_tables=True)
    for k in want:
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k
    perm = rng.permutation(Cn)                                     # cluster c becomes perm[c]
    moved = engine.links_stratified(a, b, np.where(lab >= 0, perm[np.maximum(lab, 0)], -1), Cn, want_tables=True)
    for k in ("mi", "poly", "counts", "fixed"):
        assert np.ascontiguousarray(moved[k][:, perm]).tobytes() == np.asarray(want[k]).tobytes(), k
    assert moved["neff"][perm].tobytes() == want["neff"].tobytes() and moved["mi_all"].tobytes() == want["mi_all"].tobytes()


def test_stratified_refusals_leave_the_context_usable():
    rng = np.random.default_rng(3)
    Ls, N = 30, 65
    st = random_states(rng, Ls, N)
    lab = rng.integers(0, 3, N).astype(np.int32)
    a, b = some_pairs(rng, Ls, 5)
    lib = L.lib()
    with Engine(0) as eng:
        def refused(code, a_=a, b_=b, lab_=lab, Cn=3):
            with pytest.raises(L.LdwError) as e:
                eng.links_stratified(a_, b_, lab_, Cn)
            assert e.value.code == code, (e.value.code, str(e.value))
            return str(e.value)
        with pytest.raises(L.LdwError) as e:                      # no alignment
            lab0 = np.zeros(0, dtype=np.int32)
            eng.links_stratified(a, b, lab0, 3)
        assert e.value.code == L.LDW_ERR_STATE
        eng.set_alignment(st)
        refused(L.LDW_ERR_STATE)                                   # no weights
        hdw = eng.hamming_weights(9)
        eng.set_weights(hdw)
        refused(L.LDW_ERR_ARG, a_=a[:0], b_=b[:0])               # K < 1
        refused(L.LDW_ERR_ARG, Cn=0)
        refused(L.LDW_ERR_ARG, Cn=65537)
        bad = lab.copy()
        bad[17] = 3
        assert "labels[17]" in refused(L.LDW_ERR_ARG, lab_=bad)
        bad[17] = -2
        assert "labels[17]" in refused(L.LDW_ERR_ARG, lab_=bad)
        refused(L.LDW_ERR_ARG, lab_=np.full(N, -1, dtype=np.int32))
        bad_a = a.copy()
        bad_a[3] = Ls
        assert "pair_a[3]" in refused(L.LDW_ERR_ARG, a_=bad_a)
        bad_b = b.copy()
        bad_b[4] = -1
        assert "pair_b[4]" in refused(L.LDW_ERR_ARG, b_=bad_b)
        import ctypes as C
        mi, mi_all, poly, neff, fb = np.zeros((5, 3)), np.zeros(5), np.zeros((5, 3), dtype=np.uint8), np.zeros(3), C.c_int(0)
        full = [L.ptr(a), L.ptr(b), 5, L.ptr(lab), 3, L.ptr(mi), L.ptr(mi_all), L.ptr(poly), L.ptr(neff), None, None, C.byref(fb)]
        for k in (0, 1, 3, 5, 6, 7, 8, 11):
            args = list(full)
            args[k] = None
            assert lib.ldw_links_stratified(eng._ctx, *args) == L.LDW_ERR_ARG, k
        res = eng.links_stratified(a, b, lab, 3, want_tables=True)
        check_stratified(res, R.links_stratified(st, hdw, a, b, lab, 3), "after the refusals")


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------------
def test_sequence_clusters_then_link_lineage_mi_on_a_synthetic_alignment(tmp_path):
    import pandas as pd
    syn = synth_alignment(2000, 300)
    st = np.ascontiguousarray(syn["states"])
    names = [f"seq{k}" for k in range(300)]
    snp = SnpDat.from_states(st, syn["POS"], float(syn["g"]), seq_names=names)
    rng = np.random.default_rng(8)
    a, b = some_pairs(rng, 2000, 40)
    links = pd.DataFrame({"pos1": syn["POS"][a], "pos2": syn["POS"][b], "MI": rng.random(40)})
    ref_lab, ref_n = R.seq_clusters(st, [200])
    assert ref_n[0] == 14 and sorted(np.bincount(ref_lab[0]).tolist(), reverse=True)[:5] == [96, 49, 33, 25, 20]
    with Engine(0) as eng:
        eng.set_alignment(st)
        clu = G.sequence_clusters(snp, engine=eng, alignment_resident=True)
        assert clu.thresh == 200 and clu.seq_names == names and np.array_equal(clu.labels, ref_lab[0]) and clu.sizes.tolist() == np.bincount(ref_lab[0]).tolist()
        both = G.sequence_clusters(snp, snps=[200, 0], min_size=20, small="pool", engine=eng, alignment_resident=True)
        assert sorted(both[0].sizes[:-1].tolist(), reverse=True) == [96, 49, 33, 25, 20] and both[0].sizes[-1] == 300 - 223 and both[1].sizes.tolist() == [300]
        out = tmp_path / "lineage.tsv"
        df, mi = G.link_lineage_mi(links, clu, snp, engine=eng, alignment_resident=True, per_cluster=True, out_path=out)
        big = G.link_lineage_mi(links, both[0].frame(), snp, engine=eng, alignment_resident=True, weights_resident=True)
    hdw = orc.hamming_weights(st, 0.1)
    ref = R.links_stratified(st, hdw, a, b, ref_lab[0], 14)
    cols = R.summary_columns(ref["mi"], ref["mi_all"], ref["poly"], ref["neff"])
    assert list(df.columns) == ["pos1", "pos2", "MI", "mi_all", "mi_within", "within_frac", "n_poly", "top_cluster", "top_share"]
    assert df["pos1"].tolist() == links["pos1"].tolist() and df["MI"].tolist() == links["MI"].tolist() and mi.shape == (40, 14)
    assert np.abs(mi - ref["mi"]).max() < MI_TIGHT and np.abs(df["mi_all"].to_numpy() - ref["mi_all"]).max() < MI_TIGHT
    assert np.abs(df["mi_within"].to_numpy() - cols["mi_within"]).max() < MI_TIGHT
    assert np.array_equal(df["n_poly"].to_numpy(), cols["n_poly"]) and np.array_equal(df["top_cluster"].to_numpy(), cols["top_cluster"])
    # a ratio w / a of two values known within MI_TIGHT each is known within MI_TIGHT (1 + |w / a|) / |a|
    tot = (ref["mi"] * ref["neff"]).sum(axis=1) / ref["neff"].sum()
    for name, den in (("within_frac", ref["mi_all"]), ("top_share", tot)):
        got, want = df[name].to_numpy(), cols[name]
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        ok = ~np.isnan(want)
        assert np.all(np.abs(got[ok] - want[ok]) <= MI_TIGHT * (1.0 + np.abs(want[ok])) / np.abs(den[ok])), name
    back = pd.read_csv(out, sep="\t")
    assert list(back.columns) == list(df.columns) and len(back) == 40 and np.allclose(back["mi_within"], df["mi_within"], rtol=1e-12, atol=0)
    # six clusters by name from the pooled frame: the same MI over all, since every sequence is labelled in both
    assert np.abs(big["mi_all"].to_numpy() - ref["mi_all"]).max() < MI_TIGHT
