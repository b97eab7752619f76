"""GPU: the permutation test for links (ldw_links_permuted) against the numpy restatement tests/perm_ref.py (pytest -m gpu).  Orders and
tables are compared with array_equal, MI within MI_TIGHT; counts and maxima are checked against the device's own null values, exactly."""
import ctypes as C

import numpy as np
import pytest

import caller_stream_job as J
import perm_ref as R
from ldweaver_amd import _lib as L
from ldweaver_amd import lineage as G
from ldweaver_amd.engine import Engine
from ldweaver_amd.snpdat import SnpDat
from test_lineage_host import planted

pytestmark = pytest.mark.gpu

MI_TIGHT = 1e-10       # what the 40-bit fixed-point weights deliver
HOOKS = ("LDW_PERM_BATCH", "LDW_PERM_CHUNK", "LDW_PERM_LDS")
LS = 12


@pytest.fixture(autouse=True)
def no_hooks(monkeypatch):
    for name in HOOKS:
        monkeypatch.delenv(name, raising=False)


def random_states(rng, N, Ls=LS):
    """States 0..4 (N among them); SNP 0 monomorphic, SNP 1 monomorphic in another state, SNP 2 biallelic."""
    st = rng.choice(5, size=(Ls, N), p=[0.4, 0.3, 0.15, 0.1, 0.05]).astype(np.uint8)
    st[0], st[1] = 1, 4
    st[2] = rng.integers(0, 2, N)
    return st


def some_pairs(rng, K, Ls=LS):
    """Both monomorphic (a == b, and two SNPs), monomorphic on either side, a == b polymorphic, one pair twice, then random ones."""
    fixed = [(0, 0), (0, 1), (0, 5), (5, 1), (3, 3), (7, 9), (7, 9), (2, 6)]
    a, b = [p[0] for p in fixed[:K]], [p[1] for p in fixed[:K]]
    while len(a) < K:
        a.append(int(rng.integers(Ls))), b.append(int(rng.integers(Ls)))
    return np.asarray(a, dtype=np.int32), np.asarray(b, dtype=np.int32)


def with_left_out(rng, lab_p):
    """labels [N] from the labels of the P labelled sequences: N = P + 3, a sequence left out first, last and somewhere between."""
    P = len(lab_p)
    out = np.full(P + 3, -1, dtype=np.int32)
    keep = np.ones(P + 3, dtype=bool)
    keep[[0, P + 2, 1 + int(rng.integers(P + 1))]] = False
    out[keep] = lab_p
    return out


def partitions(rng, P):
    """(name, labels of the P labelled sequences, C)."""
    zipf = lambda n: rng.choice(n, size=P, p=(1.0 / (1.0 + np.arange(n))) / (1.0 / (1.0 + np.arange(n))).sum())
    hole = zipf(6)
    hole[hole >= 2] += 1                                           # label 2 has no member, nor has the last one
    return (("singletons", rng.permutation(P), P), ("one", np.zeros(P, dtype=np.int64), 1), ("twos", rng.permutation(np.arange(P) // 2), (P + 1) // 2),
            ("zipf", zipf(6), 6), ("hole", hole, 8))


def run(eng, a, b, lab, Cn, B, seed):
    return eng.links_permuted(a, b, lab, B, seed=seed, C=Cn, want_null=True, want_tables=True, want_orders=True)


def check(eng, res, st, hdw, a, b, lab, Cn, B, seed, tag):
    """The four checks of every case, the two bit-equalities, and the lean call."""
    ref = R.links_permuted(st, hdw, a, b, lab, Cn, B, seed)
    assert res["P"] == ref["P"] and res["frac_bits"] == ref["frac_bits"] and res["n_perm"] == B, tag
    assert res["orders"].shape == ref["orders"].shape and np.array_equal(res["orders"], ref["orders"]), tag                  # 1
    assert res["fixed"].shape == ref["fixed"].shape and np.array_equal(res["fixed"], ref["fixed"]), tag                     # 2
    err = max(float(np.abs(res["null"] - ref["null"]).max()), float(np.abs(res["mi_obs"] - ref["mi_obs"]).max()))
    print(tag, f"max |MI - reference| = {err:.3e}")
    assert np.isfinite(res["null"]).all() and err < MI_TIGHT, (tag, err)                                                       # 3
    assert res["n_ge"].dtype == np.int32 and np.array_equal(res["n_ge"], (res["null"] >= res["mi_obs"][:, None]).sum(axis=1)), tag   # 4
    assert np.array_equal(res["null_max"], res["null"].max(axis=1)), tag
    strat = eng.links_stratified(a, b, lab, Cn)
    assert res["mi_obs"].tobytes() == strat["mi_all"].tobytes(), tag
    same = (res["fixed"] == ref["fixed_obs"][:, None]).all(axis=(2, 3))
    assert np.array_equal(res["null"][same], np.broadcast_to(res["mi_obs"][:, None], same.shape)[same]), tag
    lean = eng.links_permuted(a, b, lab, B, seed=seed, C=Cn)
    assert set(lean) == {"mi_obs", "n_ge", "null_max", "P", "n_perm", "frac_bits"}, tag
    for k in ("mi_obs", "n_ge", "null_max"):
        assert lean[k].tobytes() == res[k].tobytes(), (tag, k)
    return ref, same


@pytest.mark.parametrize("P", (1, 2, 63, 64, 65, 257, 300))
def test_orders_tables_and_mi_for_every_partition(engine, P):
    rng = np.random.default_rng(P)
    st = random_states(rng, P + 3)
    hdw = 1.0 / rng.integers(1, 12, P + 3)
    engine.set_alignment(st)
    engine.set_weights(hdw)
    a, b = some_pairs(rng, 9)
    for name, lab_p, Cn in partitions(rng, P):
        lab = with_left_out(rng, lab_p)
        for B in (37,) + ((1,) if name == "zipf" else ()):
            res = run(engine, a, b, lab, Cn, B, 11)
            ref, same = check(engine, res, st, hdw, a, b, lab, Cn, B, 11, (P, name, B))
            if name == "singletons":
                assert same.all() and np.all(res["n_ge"] == B) and np.array_equal(res["orders"], np.tile(R.order0(lab), (B, 1)))
            assert not res["mi_obs"][:2].any() and not res["null"][:2].any()          # both SNPs monomorphic: 0 outright
            assert res["null"][5].tobytes() == res["null"][6].tobytes()                 # one pair twice
        t = engine.last_timing()
        assert t["gemm_ms"] > 0 and t["epilogue_ms"] > 0 and t["select_ms"] > 0 and abs(t["gemm_ms"] + t["epilogue_ms"] + t["select_ms"] - t["total_ms"]) < 1e-3


def test_the_weight_stays_with_the_sequence_and_with_the_first_snp(engine):
    """A cluster of two sequences with different weights and different b-states: weights that travelled with b would swap the two cells' sums."""
    st = np.array([[1, 1, 0, 0], [2, 3, 0, 2]], dtype=np.uint8)
    hdw = np.array([1.0, 0.25, 0.5, 0.0625])
    lab = np.array([0, 0, 1, 2], dtype=np.int32)
    engine.set_alignment(st)
    engine.set_weights(hdw)
    a, b = np.array([0], dtype=np.int32), np.array([1], dtype=np.int32)
    res = run(engine, a, b, lab, 3, 64, 5)
    check(engine, res, st, hdw, a, b, lab, 3, 64, 5, "two weights")
    swapped = res["orders"][:, 0] == 1
    assert swapped.any() and not swapped.all()
    V = res["fixed"][0][~swapped][0]
    assert V[1, 2] == 4 * V[1, 3] > 0                              # (the first sequence's weight is four times the second's)
    assert np.all(res["fixed"][0][swapped][:, 1, 3] == V[1, 2]) and np.all(res["fixed"][0][swapped][:, 1, 2] == V[1, 3])
    assert len(np.unique(res["null"][0])) == 2 and res["n_ge"][0] == (res["null"][0] >= res["mi_obs"][0]).sum()


def test_batches_pair_chunks_and_kernel_forms_give_the_same_bytes(engine, monkeypatch):
    rng = np.random.default_rng(21)
    P, B = 130, 150
    st = random_states(rng, P + 3)
    hdw = 1.0 / rng.integers(1, 12, P + 3)
    engine.set_alignment(st)
    engine.set_weights(hdw)
    a, b = some_pairs(rng, 11)
    lab = with_left_out(rng, partitions(rng, P)[3][1])
    want = run(engine, a, b, lab, 6, B, 7)
    check(engine, want, st, hdw, a, b, lab, 6, B, 7, "default")
    for name, values in (("LDW_PERM_BATCH", (1, 5, 64)), ("LDW_PERM_CHUNK", (1, 4)), ("LDW_PERM_LDS", (1, 2))):
        for v in values:
            monkeypatch.setenv(name, str(v))
            got = run(engine, a, b, lab, 6, B, 7)
            for k in want:
                assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (name, v, k)
            lean = engine.links_permuted(a, b, lab, B, seed=7, C=6)
            for k in ("mi_obs", "n_ge", "null_max"):
                assert lean[k].tobytes() == want[k].tobytes(), (name, v, k)
        monkeypatch.delenv(name)
    monkeypatch.setenv("LDW_PERM_BATCH", "7")                      # all three at once
    monkeypatch.setenv("LDW_PERM_CHUNK", "3")
    monkeypatch.setenv("LDW_PERM_LDS", "1")
    got = run(engine, a, b, lab, 6, B, 7)
    for k in want:
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k


def test_two_seeds_differ_and_one_seed_twice_is_identical(engine):
    rng = np.random.default_rng(22)
    P = 90
    st = random_states(rng, P + 3)
    hdw = 1.0 / rng.integers(1, 5, P + 3)
    engine.set_alignment(st)
    engine.set_weights(hdw)
    a, b = some_pairs(rng, 8)
    lab = with_left_out(rng, partitions(rng, P)[3][1])
    one, again, other = run(engine, a, b, lab, 6, 20, 1), run(engine, a, b, lab, 6, 20, 1), run(engine, a, b, lab, 6, 20, (1 << 64) - 1)
    for k in one:
        assert np.asarray(one[k]).tobytes() == np.asarray(again[k]).tobytes(), k
    assert not np.array_equal(one["orders"], other["orders"]) and not np.array_equal(one["null"], other["null"])
    assert one["mi_obs"].tobytes() == other["mi_obs"].tobytes()
    check(engine, other, st, hdw, a, b, lab, 6, 20, (1 << 64) - 1, "largest seed")
    assert np.array_equal(run(engine, a, b, lab, 6, 5, 1)["null"], one["null"][:, :5])          # replicate r does not depend on B


@pytest.mark.parametrize("N,Ls,K,B", ((70000, 8, 3, 4), (7000, 4, 2, 3)))
def test_many_sequences_where_the_staged_rows_fill_the_lds(engine, N, Ls, K, B):
    """70 000 sequences: the two state arrays take 140 of the 160 KiB, the weights are read from global memory; 7 000: weights and states take 70 KiB, past
    the 64 KiB a kernel gets without asking."""
    rng = np.random.default_rng(N)
    st = rng.choice(5, size=(Ls, N), p=[0.5, 0.3, 0.1, 0.07, 0.03]).astype(np.uint8)
    hdw = 1.0 / rng.integers(1, 40, N)
    lab = rng.integers(0, 5, N).astype(np.int32)
    engine.set_alignment(st)
    engine.set_weights(hdw)
    a, b = rng.integers(0, Ls, K).astype(np.int32), rng.integers(0, Ls, K).astype(np.int32)
    res = run(engine, a, b, lab, 5, B, 12345)
    check(engine, res, st, hdw, a, b, lab, 5, B, 12345, (N, Ls))
    assert res["P"] == N


def test_refusals_leave_the_context_usable():
    rng = np.random.default_rng(3)
    N = 65
    st = random_states(rng, N)
    lab = rng.integers(0, 3, N).astype(np.int32)
    a, b = some_pairs(rng, 5)
    lib = L.lib()
    with Engine(0) as eng:
        def refused(code, a_=a, b_=b, lab_=lab, Cn=3, B=10):
            with pytest.raises(L.LdwError) as e:
                eng.links_permuted(a_, b_, lab_, B, seed=1, C=Cn)
            assert e.value.code == code, (e.value.code, str(e.value))
            assert "ldw_links_permuted" in str(e.value)
            return str(e.value)
        with pytest.raises(L.LdwError) as e:                      # no alignment
            eng.links_permuted(a, b, np.zeros(0, dtype=np.int32), 10, C=3)
        assert e.value.code == L.LDW_ERR_STATE
        eng.set_alignment(st)
        assert "weights" in refused(L.LDW_ERR_STATE)              # no weights
        hdw = 1.0 / rng.integers(1, 7, N)
        eng.set_weights(hdw)
        refused(L.LDW_ERR_ARG, a_=a[:0], b_=b[:0])               # K < 1
        for B in (0, -1, (1 << 24) + 1):
            assert "replicates" in refused(L.LDW_ERR_ARG, B=B)
        refused(L.LDW_ERR_ARG, Cn=0)
        refused(L.LDW_ERR_ARG, Cn=65537)
        bad = lab.copy()
        bad[17] = 3
        assert "labels[17]" in refused(L.LDW_ERR_ARG, lab_=bad)
        bad[17] = -2
        assert "labels[17]" in refused(L.LDW_ERR_ARG, lab_=bad)
        refused(L.LDW_ERR_ARG, lab_=np.full(N, -1, dtype=np.int32))
        bad_a = a.copy()
        bad_a[3] = LS
        assert "pair_a[3]" in refused(L.LDW_ERR_ARG, a_=bad_a)
        bad_b = b.copy()
        bad_b[4] = -1
        assert "pair_b[4]" in refused(L.LDW_ERR_ARG, b_=bad_b)
        mi, n_ge, mx, p, fb = np.zeros(5), np.zeros(5, dtype=np.int32), np.zeros(5), C.c_int64(0), C.c_int(0)
        full = [L.ptr(a), L.ptr(b), 5, L.ptr(lab), 3, 10, 1, L.ptr(mi), L.ptr(n_ge), L.ptr(mx), None, None, None, C.byref(p), C.byref(fb)]
        for k in (0, 1, 3, 7, 8, 9, 13, 14):
            args = list(full)
            args[k] = None
            assert lib.ldw_links_permuted(eng._ctx, *args) == L.LDW_ERR_ARG, k
        assert eng.links_permuted(a[:1], b[:1], lab, 1, C=3)["n_ge"].shape == (1,)                     # the smallest call
        res = run(eng, a, b, lab, 3, 10, 1)
        check(eng, res, st, hdw, a, b, lab, 3, 10, 1, "after the refusals")
        assert np.array_equal(eng.get_alignment(), st)


def test_on_a_caller_owned_stream():
    rng = np.random.default_rng(31)
    P = 129
    st = random_states(rng, P + 3)
    hdw = 1.0 / rng.integers(1, 9, P + 3)
    a, b = some_pairs(rng, 9)
    lab = with_left_out(rng, partitions(rng, P)[3][1])
    cs = J.CallerStream("not_current")
    try:
        with Engine(0, stream=cs.handle) as eng:
            eng.set_alignment(st)
            eng.set_weights(hdw)
            res = run(eng, a, b, lab, 6, 40, 9)
            check(eng, res, st, hdw, a, b, lab, 6, 40, 9, "caller stream")
        assert cs.works()
    finally:
        cs.close()


def test_link_permutation_test_on_the_planted_lineages(tmp_path):
    import pandas as pd
    st, lin = planted(np.random.default_rng(7))
    snp = SnpDat.from_states(st, np.arange(1, 7) * 10, 100.0, seq_names=[f"s{k}" for k in range(200)])
    links = pd.DataFrame({"pos1": [10, 50, 30], "pos2": [20, 60, 40], "MI": [0.6, 0.5, 0.4]})
    hdw = np.ones(200)
    B = 999
    with Engine(0) as eng:
        eng.set_alignment(st)
        free, null = G.link_permutation_test(links, None, snp, n_perm=B, seed=0, hdw=hdw, engine=eng, alignment_resident=True, return_null=True)
        out = tmp_path / "perm.tsv"
        within = G.link_permutation_test(links, lin, snp, n_perm=B, seed=0, hdw=hdw, engine=eng, alignment_resident=True, out_path=out)
        ham = G.link_permutation_test(links, lin, snp, n_perm=20, engine=eng, alignment_resident=True)       # the Hamming weights at 0.1
    assert list(within.columns) == ["pos1", "pos2", "MI", "mi_all", "perm_ge", "perm_p", "null_max", "n_perm"] and null.shape == (3, B)
    # lineage markers: unrestricted p = 1 / (1 + B); within the lineages every replicate's table is the observed one
    assert free["perm_ge"][0] == 0 and free["perm_p"][0] == 1.0 / (1 + B) and within["perm_ge"][0] == B and within["perm_p"][0] == 1.0
    assert within["null_max"][0] == within["mi_all"][0] and within["perm_p"][1] <= 0.01 and free["perm_p"][1] <= 0.01
    a, b = [0, 4, 2], [1, 5, 3]
    for df, lab, Cn in ((free, np.zeros(200, dtype=np.int64), 1), (within, lin, 2)):
        ref = R.links_permuted(st, hdw, a, b, lab, Cn, B, 0)
        assert np.abs(df["mi_all"].to_numpy() - ref["mi_obs"]).max() < MI_TIGHT and np.abs(df["null_max"].to_numpy() - ref["null_max"]).max() < MI_TIGHT
        # a count may differ from the reference's only where a replicate's MI lies within MI_TIGHT of the observed one without being it
        near = (np.abs(ref["null"] - ref["mi_obs"][:, None]) < MI_TIGHT) & (ref["null"] != ref["mi_obs"][:, None])
        assert np.all(np.abs(df["perm_ge"].to_numpy() - ref["n_ge"]) <= near.sum(axis=1))
    assert np.array_equal(free["perm_ge"].to_numpy(), (null >= free["mi_all"].to_numpy()[:, None]).sum(axis=1))
    back = pd.read_csv(out, sep="\t")
    assert list(back.columns) == list(within.columns) and np.allclose(back["perm_p"], within["perm_p"], rtol=1e-12, atol=0)
    assert ham["n_perm"].tolist() == [20] * 3 and ham["perm_ge"][0] == 20
