"""GPU: ldw_mi_snp_summary (Engine.mi_snp_summary, ldweaver_amd.background; pytest -m gpu) on the bundled sample alignment in blocks of 500 —
against the numpy statement tests/snpsum_ref.py applied to the engine's own dense blocks (exactly), against the pass's own pair counts, against the oracle's
MI (n (MI_TIGHT + 2^-41) per SNP and class) — and on the planted example of the average product correction through snp_background and link_apc."""
import os

import numpy as np
import pandas as pd
import pytest

import c_oracle
import caller_stream_job as J
import snpsum_ref as R
from ldweaver_amd import _lib as L
from ldweaver_amd import background as B
from ldweaver_amd import mi as MIH
from ldweaver_amd import plots
from ldweaver_amd.engine import Engine
from ldweaver_amd.snpdat import SnpDat

pytestmark = pytest.mark.gpu

MI_TIGHT = 1e-10       # what the 40-bit fixed-point weights deliver, the bound on each value
BLK = 500              # 1268 SNPs: blocks of 500, 500 and 268 — diagonal, square off-diagonal and ragged off-diagonal pairs
SR_DIST = 3000.0
NSNP = 1268
QUIRKS = (L.QUIRK_REFERENCE, L.QUIRK_INTENDED)


def setup(eng, d, POS=None):
    eng.set_engine(L.ENGINE_MFMA)
    eng.set_alignment(d["states"])
    eng.set_weights(d["hdw"])
    eng.set_snp_meta(d["r"], d["uqe"], d["POS"] if POS is None else POS, d["paint"], d["g"])


class Problem:
    """The sample's blocks; the engine's dense blocks per quirk mode and the oracle's, each made once and never changed; the thresholds of nge, taken from
    the values themselves."""

    def __init__(self, sample):
        self.d = sample
        self.blocks = np.ascontiguousarray(MIH.make_blocks(NSNP, BLK), dtype=np.int32)
        assert len(self.blocks) == 6
        self.lists = [(np.arange(fs - 1, fe), np.arange(ts - 1, te), fs == ts and fe == te) for fs, fe, ts, te in self.blocks]
        self.shuffled = np.random.default_rng(3).permutation(sample["POS"]).astype(np.int32)
        self._dense, self._oracle, self._thr = {}, {}, {}

    def dense(self, eng, quirk):
        if quirk not in self._dense:
            self._dense[quirk] = [eng.mi_block(fi, ti, quirk=quirk) for fi, ti, _ in self.lists]
            v = np.sort(self._dense[quirk][1].ravel())
            self._thr[quirk] = (float(v[int(0.99 * len(v))]), float(v[int(0.9 * len(v))]))     # values of the block: the comparison is closed
        return self._dense[quirk]

    def thr(self, eng, quirk):
        self.dense(eng, quirk)
        return self._thr[quirk]

    def oracle(self, quirk):
        if quirk not in self._oracle:
            d = self.d
            if quirk == L.QUIRK_REFERENCE:      # the reference's reading of RXY depends on the block's geometry: block by block
                self._oracle[quirk] = [c_oracle.mi_block(d["states"], d["hdw"], d["r"], d["uqe"], fi, ti) for fi, ti, _ in self.lists]
            else:                               # one square block over every SNP: there RXY is r r' (tests/test_gpu_parity.py)
                idx = np.arange(NSNP)
                full = c_oracle.mi_block(d["states"], d["hdw"], d["r"], d["uqe"], idx, idx)
                self._oracle[quirk] = [full[np.ix_(fi, ti)] for fi, ti, _ in self.lists]
        return self._oracle[quirk]

    def statement(self, blocks_mi, POS, thr):
        """snpsum_ref.snp_summary of the given dense blocks, both sides of every block folded into the SNPs' totals."""
        tot, npairs, refused = R.empty_total(NSNP), np.zeros(2, np.int64), 0
        for M, (fi, ti, diag) in zip(blocks_mi, self.lists):
            rows, cols, n, ref = R.snp_summary(M, POS[fi], POS[ti], self.d["g"], diag, SR_DIST, thr)
            R.fold(tot, rows, fi)
            R.fold(tot, cols, ti)
            npairs += n
            refused += ref
        return tot, npairs, refused


@pytest.fixture(scope="module")
def prob(sample):
    return Problem(sample)


@pytest.mark.parametrize("quirk", QUIRKS)
@pytest.mark.parametrize("order", ("ascending", "shuffled"))
def test_a_summary_equals_the_statement_on_the_engines_own_blocks(engine, prob, quirk, order):
    POS = prob.d["POS"] if order == "ascending" else prob.shuffled
    setup(engine, prob.d, POS)
    thr = prob.thr(engine, quirk)
    ref, ref_np, ref_refused = prob.statement(prob.dense(engine, quirk), POS, thr)
    got = engine.mi_snp_summary(prob.blocks, SR_DIST, thr, quirk=quirk)
    for k in ("n", "sumq", "nge"):
        assert got[k].dtype == np.int64 and got[k].shape == (2, NSNP) and np.array_equal(got[k], ref[k]), (k, np.argwhere(got[k] != ref[k])[:5])
    assert R.same_bits(got["max"], ref["max"])
    assert ref["nge"][0].sum() > 0 and ref["nge"][1].sum() > 0
    # every SNP pair but the local diagonals of the three off-diagonal blocks, which the reference drops (R/computePairwiseMI.R:306-310)
    assert np.array_equal(got["npairs"], ref_np) and int(got["npairs"].sum()) == NSNP * (NSNP - 1) // 2 - 1036
    assert np.array_equal(got["n"].sum(axis=1), 2 * got["npairs"])
    rep = engine.snp_summary_report()
    assert rep["blocks"] == 6 and rep["patches"] > 0 and rep["refused"] == 0 == ref_refused and rep["off_class"] == 0
    t = engine.last_timing()
    assert t["gemm_ms"] > 0 and t["epilogue_ms"] > 0 and t["select_ms"] == 0 and abs(t["gemm_ms"] + t["epilogue_ms"] - t["total_ms"]) < 1e-6
    lean = np.zeros((2, NSNP), dtype=np.int64), np.zeros((2, NSNP), dtype=np.int64), np.zeros(2, dtype=np.int64)      # max_out and nge_out may be NULL
    th = np.asarray(thr, dtype=np.float64)
    L.check(L.lib().ldw_mi_snp_summary(engine._ctx, L.ptr(prob.blocks), 6, int(quirk), SR_DIST, L.ptr(th), L.ptr(lean[0]), L.ptr(lean[1]), None, None, L.ptr(lean[2])))
    assert np.array_equal(lean[0], ref["n"]) and np.array_equal(lean[1], ref["sumq"]) and np.array_equal(lean[2], ref_np)


@pytest.mark.parametrize("quirk", QUIRKS)
def test_b_sums_against_the_oracle(engine, prob, quirk):
    """Per SNP and class |sumq / 2^40 - sum of the oracle's MI| <= n (MI_TIGHT + 2^-41): MI_TIGHT bounds each value, 2^-41 is the half-unit of the fixed
    point.  No slack beyond that and no SNP left out; the oracle's sum is taken in extended precision."""
    setup(engine, prob.d)
    got = engine.mi_snp_summary(prob.blocks, SR_DIST, quirk=quirk)
    POS = prob.d["POS"]
    tot = np.zeros((2, NSNP), dtype=np.longdouble)
    cnt = np.zeros((2, NSNP), dtype=np.int64)
    from decay_ref import circ_len, pair_mask
    for M, (fi, ti, diag) in zip(prob.oracle(quirk), prob.lists):
        m = pair_mask(len(fi), len(ti), diag)
        cls = np.where(circ_len(POS[ti][None, :], POS[fi][:, None], prob.d["g"]) <= SR_DIST, 0, 1)
        for c in (0, 1):
            hit = m & (cls == c)
            v = np.where(hit, M, 0.0).astype(np.longdouble)
            tot[c, fi] += v.sum(axis=1)
            tot[c, ti] += v.sum(axis=0)
            cnt[c, fi] += hit.sum(axis=1)
            cnt[c, ti] += hit.sum(axis=0)
    assert np.array_equal(cnt, got["n"])
    err = np.abs(got["sumq"].astype(np.longdouble) / np.longdouble(2.0 ** 40) - tot)
    bound = got["n"] * (MI_TIGHT + 2.0 ** -41)
    print("worst |sum - oracle| / bound:", float((err[got["n"] > 0] / bound[got["n"] > 0]).max()), "worst per value:", float((err[got["n"] > 0] / got["n"][got["n"] > 0]).max()))
    assert (err <= bound).all(), (np.argwhere(err > bound)[:5], err.max())
    assert (got["n"].sum(axis=0) > 0).all()                                    # every SNP has partners


@pytest.mark.parametrize("order", ("ascending", "shuffled"))
def test_c_the_pair_counts_are_the_passes_and_the_link_tables_stay(engine, prob, order):
    d = prob.d
    POS = d["POS"] if order == "ascending" else prob.shuffled
    setup(engine, d, POS)
    approx = MIH.lr_links_approx(POS, d["g"], SR_DIST)
    engine.reset_speculation()
    engine.mi_all_pairs(prob.blocks, SR_DIST, 2000.0, approx)
    stats = engine.block_stats()
    before = (engine.links_count(0), engine.links_count(1), engine.links(0), engine.links(1))
    got = engine.mi_snp_summary(prob.blocks, SR_DIST)
    assert int(got["npairs"][0]) == int(stats["n_sr"].sum()) and int(got["npairs"][1]) == int(stats["n_lr_total"].sum())
    assert np.array_equal(got["n"].sum(axis=1), 2 * got["npairs"]) and not got["nge"].any()
    after = (engine.links_count(0), engine.links_count(1), engine.links(0), engine.links(1))
    assert before[:2] == after[:2] and before[0] > 0 and before[1] > 0
    for tb, ta in zip(before[2:], after[2:]):
        for x, y in zip(tb, ta):
            assert np.array_equal(x, y)
    again = engine.block_stats()
    assert all(np.array_equal(stats[k], again[k]) for k in stats)


def test_d_on_a_caller_owned_stream(engine, prob):
    setup(engine, prob.d)
    ref = engine.mi_snp_summary(prob.blocks, SR_DIST, (0.05, 0.05))
    with J.caller_stream("not_current") as cs:
        with Engine(0, stream=cs.handle) as eng:
            setup(eng, prob.d)
            got = eng.mi_snp_summary(prob.blocks, SR_DIST, (0.05, 0.05))
        assert cs.works()
    assert all(np.array_equal(got[k], ref[k]) for k in ("n", "sumq", "nge", "npairs")) and R.same_bits(got["max"], ref["max"])


def test_states_and_block_refusals(engine, prob):
    with Engine(0) as eng:
        with pytest.raises(L.LdwError) as e:                                # nothing set
            eng.mi_snp_summary(prob.blocks, SR_DIST)
        assert e.value.code == L.LDW_ERR_STATE
        eng.set_alignment(prob.d["states"])
        eng.set_weights(prob.d["hdw"])
        with pytest.raises(L.LdwError) as e:                                # no SNP meta data
            eng.mi_snp_summary(prob.blocks, SR_DIST)
        assert e.value.code == L.LDW_ERR_STATE
        assert "ldw_mi_snp_summary" in str(e.value)                         # the shared walk speaks under its caller's name
    setup(engine, prob.d)
    for bad in ([1, 500, 400, 900], [1, 500, 1, 400], [0, 500, 0, 500], [1, 1269, 1, 1269], [500, 1, 500, 1]):
        with pytest.raises(L.LdwError) as e:
            engine.mi_snp_summary(np.array([bad], dtype=np.int32), SR_DIST)
        assert e.value.code == L.LDW_ERR_ARG and "ldw_mi_snp_summary" in str(e.value), bad
    for sr in (-1.0, np.nan):
        with pytest.raises(L.LdwError) as e:
            engine.mi_snp_summary(prob.blocks, sr)
        assert e.value.code == L.LDW_ERR_ARG
    got = engine.mi_snp_summary(np.array([[501, 1000, 1, 500]], dtype=np.int32), np.inf)     # disjoint, the to side first: a legal block; every pair short range
    assert got["npairs"].tolist() == [500 * 500 - 500, 0] and not got["n"][:, 1000:].any()


def test_the_planted_example_through_snp_background_and_link_apc(engine, tmp_path):
    st, pos, g, sr, markers, (pa, pb) = R.planted_apc()
    snp = SnpDat.from_states(st, pos, g)
    out, png = tmp_path / "background.tsv", tmp_path / "background.png"
    bg = B.snp_background(snp, np.ones(st.shape[1]), sr_dist=sr, thr=(np.inf, 0.3), engine=engine, out_path=str(out), plot_path=str(png))
    assert bg.npairs.tolist() == [0, 120 * 119 // 2] and not bg.n[0].any() and (bg.n[1] == 119).all() and bg.sr_dist == sr and bg.g == g
    idx = np.arange(len(st))
    M = engine.mi_block(idx, idx)                                              # the values the summary saw: the engine still holds the problem
    a, b = np.tril_indices(len(st), -1)
    links = B.link_apc(pd.DataFrame({"pos1": pos[a], "pos2": pos[b], "MI": M[a, b]}), bg, snp)
    assert len(links) == 7140 and np.array_equal(links["pos1"], pos[a]) and np.array_equal(links["MI"], M[a, b])
    is_marker = np.isin(a, markers) & np.isin(b, markers)
    p = int(np.flatnonzero((a == max(pa, pb)) & (b == min(pa, pb)))[0])
    raw, apc = links["MI"].to_numpy(), links["mi_apc"].to_numpy()
    print("planted raw", raw[p], "marker raw min", raw[is_marker].min(), "planted mi_apc", apc[p], "marker mi_apc max", apc[is_marker].max())
    assert is_marker.sum() == 780 and raw[is_marker].min() > raw[p]             # by raw MI all 780 marker pairs rank above the planted pair
    assert int(np.argmax(apc)) == p                                             # by mi_apc the planted pair ranks first
    assert apc[is_marker].max() < 0.5 * apc[p]
    assert set(bg.hubs("lr", 40)["snp"]) == set(markers.tolist())               # the hubs are the markers
    assert bg.nge[1].sum() == 2 * int((M[a, b] >= 0.3).sum())
    fr = bg.frame()
    back = pd.read_csv(out, sep="\t", float_precision="round_trip")
    assert list(back.columns) == list(fr.columns) and len(back) == len(fr) == 120
    for c in fr.columns:      # the native writer prints R's 15 significant digits: equal to that precision, integers exactly, NA where a class has no partner
        x, y = fr[c].to_numpy(dtype=np.float64), back[c].to_numpy(dtype=np.float64)
        assert np.array_equal(np.isnan(x), np.isnan(y)) and np.allclose(x[~np.isnan(x)], y[~np.isnan(y)], rtol=1e-14, atol=0), c
    W, H = plots.CANVAS[L.PLOT_FIT]
    with open(png, "rb") as f:
        head = f.read(24)
    assert head[:8] == b"\x89PNG\r\n\x1a\n" and int.from_bytes(head[16:20], "big") == W and int.from_bytes(head[20:24], "big") == H
    assert os.path.getsize(png) > 1000
