"""GPU: ldw_mi_score_scan and ldw_mi_score_links (Engine.mi_score_scan / mi_score_links, background.apc_links; pytest -m gpu) on the bundled
sample alignment in blocks of 500 — against the numpy statement tests/scoresel_ref.py applied to the engine's own dense blocks (exactly: the score is two
stated IEEE operations on the device's own MI bits), against ldw_mi_snp_summary's pair counts — and on the planted example of the average product correction
through apc_links, whose mi_apc is compared with link_apc's within the roundings by which the two forms differ."""
import numpy as np
import pandas as pd
import pytest

import caller_stream_job as J
import scoresel_ref as S
import snpsum_ref as R
from ldweaver_amd import _lib as L
from ldweaver_amd import background as B
from ldweaver_amd import mi as MIH
from ldweaver_amd.engine import Engine
from ldweaver_amd.snpdat import SnpDat

pytestmark = pytest.mark.gpu

BLK = 500              # 1268 SNPs: blocks of 500, 500 and 268 — diagonal, square off-diagonal and ragged off-diagonal pairs
SR_DIST = 3000.0
NSNP = 1268
TOP = 500
QUIRKS = (L.QUIRK_REFERENCE, L.QUIRK_INTENDED)


def setup(eng, d, POS=None):
    eng.set_engine(L.ENGINE_MFMA)
    eng.set_alignment(d["states"])
    eng.set_weights(d["hdw"])
    eng.set_snp_meta(d["r"], d["uqe"], d["POS"] if POS is None else POS, d["paint"], d["g"])


class Problem:
    """The sample's blocks, the engine's dense blocks per quirk mode (made once, never changed) and a weight per SNP: of the size of the root of the mean MI,
    a tenth of them negative, a few zero."""

    def __init__(self, sample):
        self.d = sample
        self.blocks = np.ascontiguousarray(MIH.make_blocks(NSNP, BLK), dtype=np.int32)
        assert len(self.blocks) == 6
        self.lists = [(np.arange(fs - 1, fe), np.arange(ts - 1, te), fs == ts and fe == te) for fs, fe, ts, te in self.blocks]
        rng = np.random.default_rng(3)
        self.shuffled = rng.permutation(sample["POS"]).astype(np.int32)
        self.w = rng.uniform(0.02, 0.3, NSNP) * np.where(rng.random(NSNP) < 0.1, -1.0, 1.0)
        self.w[::97] = 0.0
        self._dense = {}

    def dense(self, eng, quirk):
        if quirk not in self._dense:
            self._dense[quirk] = [eng.mi_block(fi, ti, quirk=quirk) for fi, ti, _ in self.lists]
        return self._dense[quirk]

    def statement(self, blocks_mi, POS, mask, top):
        """The scan of every block folded into the SNPs' totals, the threshold rule, then the links and the partner minima of every block against the
        totals' bests."""
        g, w = self.d["g"], self.w
        tot = S.empty_total(NSNP)
        for M, (fi, ti, diag) in zip(blocks_mi, self.lists):
            S.fold(tot, S.scan(M, POS[fi], POS[ti], g, diag, SR_DIST, mask, w[fi], w[ti]), fi, ti)
        thr, cap = S.pick_threshold(tot["hist"], top)
        listed, partner = set(), np.full(NSNP, -1, dtype=np.int64)
        for M, (fi, ti, diag) in zip(blocks_mi, self.lists):
            lk, pf, pt = S.links(M, POS[fi], POS[ti], g, diag, SR_DIST, mask, fi, ti, w[fi], w[ti], thr, tot["best"][fi], tot["best"][ti])
            assert not listed & lk
            listed |= lk
            S.fold_partner(partner, pf, fi)
            S.fold_partner(partner, pt, ti)
        return tot, thr, cap, listed, partner


@pytest.fixture(scope="module")
def prob(sample):
    return Problem(sample)


def as_rows(got):
    return sorted(zip(got["a"].tolist(), got["b"].tolist(), got["mi"].view(np.int64).tolist(), got["score"].view(np.int64).tolist()))


@pytest.mark.parametrize("mask", (1, 2, 3))
@pytest.mark.parametrize("quirk", QUIRKS)
@pytest.mark.parametrize("order", ("ascending", "shuffled"))
def test_a_scan_and_links_equal_the_statement_on_the_engines_own_blocks(engine, prob, quirk, order, mask):
    POS = prob.d["POS"] if order == "ascending" else prob.shuffled
    setup(engine, prob.d, POS)
    ref, thr, cap, listed, partner = prob.statement(prob.dense(engine, quirk), POS, mask, TOP)
    scan = engine.mi_score_scan(prob.blocks, SR_DIST, mask, prob.w, quirk=quirk)
    assert scan["hist"].dtype == np.uint64 and np.array_equal(scan["hist"], ref["hist"]), np.flatnonzero(scan["hist"] != ref["hist"])[:5]
    assert scan["best"].shape == (NSNP,) and S.same_bits(scan["best"], ref["best"])               # every SNP
    rep = engine.score_select_report()
    assert rep["blocks"] == 6 and rep["patches"] > 0 and rep["nan_scores"] == ref["nan"] == 0
    assert int(scan["hist"].sum()) + rep["nan_scores"] == scan["npairs"] == ref["npairs"]
    summ = engine.mi_snp_summary(prob.blocks, SR_DIST, quirk=quirk)["npairs"]
    assert scan["npairs"] == int(summ[0] if mask == 1 else summ[1] if mask == 2 else summ.sum()) > 0
    assert B.pick_threshold(scan["hist"], TOP) == (thr, cap) and cap > 0
    got = engine.mi_score_links(prob.blocks, SR_DIST, mask, prob.w, thr, cap, best_in=scan["best"], quirk=quirk)
    assert got["count"] == cap == len(listed)
    assert as_rows(got) == sorted(listed)                                                          # every pair
    assert got["partner"].dtype == np.int32 and np.array_equal(got["partner"], partner)
    assert np.array_equal(got["partner"] < 0, np.isnan(ref["best"])) and (got["partner"] >= 0).any()
    t = engine.last_timing()
    assert t["gemm_ms"] > 0 and t["epilogue_ms"] > 0 and t["select_ms"] == 0 and abs(t["gemm_ms"] + t["epilogue_ms"] - t["total_ms"]) < 1e-6
    rep = engine.score_select_report()
    assert rep["blocks"] == 6 and rep["nan_scores"] == 0
    lean = engine.mi_score_links(prob.blocks, SR_DIST, mask, prob.w, thr, 0, quirk=quirk)          # a pure count, no partners
    assert lean["count"] == cap and lean["a"] is None and lean["partner"] is None
    with pytest.raises(L.LdwError) as e:
        engine.mi_score_links(prob.blocks, SR_DIST, mask, prob.w, thr, cap - 1, quirk=quirk)
    assert e.value.code == L.LDW_ERR_SIZE and e.value.count == cap


@pytest.mark.parametrize("order", ("ascending", "shuffled"))
def test_b_the_link_tables_and_block_stats_of_a_pass_stay(engine, prob, order):
    d = prob.d
    POS = d["POS"] if order == "ascending" else prob.shuffled
    setup(engine, d, POS)
    approx = MIH.lr_links_approx(POS, d["g"], SR_DIST)
    engine.reset_speculation()
    engine.mi_all_pairs(prob.blocks, SR_DIST, 2000.0, approx)
    stats = engine.block_stats()
    before = (engine.links_count(0), engine.links_count(1), engine.links(0), engine.links(1))
    scan = engine.mi_score_scan(prob.blocks, SR_DIST, 2, prob.w)
    assert scan["npairs"] == int(stats["n_lr_total"].sum())
    thr, cap = B.pick_threshold(scan["hist"], 50)
    assert engine.mi_score_links(prob.blocks, SR_DIST, 2, prob.w, thr, cap, best_in=scan["best"])["count"] == cap
    after = (engine.links_count(0), engine.links_count(1), engine.links(0), engine.links(1))
    assert before[:2] == after[:2] and before[0] > 0 and before[1] > 0
    for tb, ta in zip(before[2:], after[2:]):
        for x, y in zip(tb, ta):
            assert np.array_equal(x, y)
    again = engine.block_stats()
    assert all(np.array_equal(stats[k], again[k]) for k in stats)


def test_c_on_a_caller_owned_stream(engine, prob):
    setup(engine, prob.d)
    ref = engine.mi_score_scan(prob.blocks, SR_DIST, 3, prob.w)
    thr, cap = B.pick_threshold(ref["hist"], 100)
    ref_l = engine.mi_score_links(prob.blocks, SR_DIST, 3, prob.w, thr, cap, best_in=ref["best"])
    with J.caller_stream("not_current") as cs:
        with Engine(0, stream=cs.handle) as eng:
            setup(eng, prob.d)
            got = eng.mi_score_scan(prob.blocks, SR_DIST, 3, prob.w)
            got_l = eng.mi_score_links(prob.blocks, SR_DIST, 3, prob.w, thr, cap, best_in=got["best"])
        assert cs.works()
    assert np.array_equal(got["hist"], ref["hist"]) and S.same_bits(got["best"], ref["best"]) and got["npairs"] == ref["npairs"]
    assert as_rows(got_l) == as_rows(ref_l) and np.array_equal(got_l["partner"], ref_l["partner"])


def test_states_and_argument_refusals(engine, prob):
    with Engine(0) as eng:
        with pytest.raises(L.LdwError) as e:                                # nothing set
            eng.mi_score_scan(prob.blocks, SR_DIST, 3, np.zeros(0))
        assert e.value.code == L.LDW_ERR_STATE and "ldw_mi_score_scan" in str(e.value)
        eng.set_alignment(prob.d["states"])
        eng.set_weights(prob.d["hdw"])
        with pytest.raises(L.LdwError) as e:                                # no SNP meta data
            eng.mi_score_links(prob.blocks, SR_DIST, 3, prob.w, 0.1)
        assert e.value.code == L.LDW_ERR_STATE and "ldw_mi_score_links" in str(e.value)
    setup(engine, prob.d)
    for bad in ([1, 500, 400, 900], [0, 500, 0, 500], [1, 1269, 1, 1269]):
        with pytest.raises(L.LdwError) as e:
            engine.mi_score_scan(np.array([bad], dtype=np.int32), SR_DIST, 3, prob.w)
        assert e.value.code == L.LDW_ERR_ARG and "ldw_mi_score_scan" in str(e.value), bad
    w = prob.w.copy()
    w[777] = np.inf
    for call in (lambda: engine.mi_score_scan(prob.blocks, SR_DIST, 3, w), lambda: engine.mi_score_links(prob.blocks, SR_DIST, 3, w, 0.1)):
        with pytest.raises(L.LdwError) as e:
            call()
        assert e.value.code == L.LDW_ERR_ARG and "w[777]" in str(e.value)
    for sr, mask in ((-1.0, 3), (np.nan, 3), (SR_DIST, 0), (SR_DIST, 4)):
        with pytest.raises(L.LdwError) as e:
            engine.mi_score_scan(prob.blocks, sr, mask, prob.w)
        assert e.value.code == L.LDW_ERR_ARG
    import ctypes as C
    n, part, wv = C.c_int64(0), np.zeros(NSNP, dtype=np.int32), np.ascontiguousarray(prob.w)
    rc = L.lib().ldw_mi_score_links(engine._ctx, L.ptr(prob.blocks), 6, 0, SR_DIST, 3, L.ptr(wv), 0.1, None, 0, None, None, None, None, C.byref(n), L.ptr(part))
    assert rc == L.LDW_ERR_ARG                                                 # partner_out needs best_in
    got = engine.mi_score_scan(np.array([[501, 1000, 1, 500]], dtype=np.int32), np.inf, 1, prob.w)     # disjoint, the to side first: a legal block
    assert got["npairs"] == 500 * 500 - 500 and np.isnan(got["best"][1000:]).all() and not np.isnan(got["best"][:1000]).any()


def test_the_planted_example_through_apc_links(engine, tmp_path):
    st, pos, g, sr, markers, (pa, pb) = R.planted_apc()
    snp = SnpDat.from_states(st, pos, g)
    ones = np.ones(st.shape[1])
    out = tmp_path / "apc_links.tsv"
    links, partners = B.apc_links(snp, ones, top=10, sr_dist=sr, engine=engine, out_path=str(out))
    assert list(links.columns) == ["pos1", "pos2", "len", "MI", "bg1", "bg2", "apc", "mi_apc"] and len(links) == 10
    assert list(partners.columns) == ["pos", "best", "partner_pos", "partner_snp"] and len(partners) == 120
    lo, hi = min(pa, pb), max(pa, pb)
    assert {links["pos1"][0], links["pos2"][0]} == {float(pos[pa]), float(pos[pb])}            # row 0 is the planted pair
    assert (links["pos1"][0], links["pos2"][0]) == (float(pos[lo]), float(pos[hi]))            # pos1 the to-SNP (the column), pos2 the from-SNP
    assert (np.diff(links["mi_apc"].to_numpy()) <= 0).all() and links["mi_apc"][1] < 0.5 * links["mi_apc"][0]
    assert partners["partner_snp"][pa] == pb and partners["partner_snp"][pb] == pa and partners["partner_pos"][pa] == pos[pb]
    assert partners["best"][pa] == partners["best"][pb] == links["mi_apc"][0] and (partners["partner_snp"] >= 0).all()
    # the flow itself: the links call returns exactly the cap of the threshold rule
    bg = B.snp_background(snp, ones, sr_dist=sr, engine=engine)
    w = B.apc_weights(bg, "lr")
    blocks = MIH.make_blocks(120, 10000)
    scan = engine.mi_score_scan(blocks, sr, 2, w)
    thr, cap = B.pick_threshold(scan["hist"], 10)
    got = engine.mi_score_links(blocks, sr, 2, w, thr, cap, best_in=scan["best"])
    assert got["count"] == cap == partners.attrs["cap"] >= 10 and scan["npairs"] == 7140 and thr == partners.attrs["thr"]
    # against link_apc on the same rows: mean mean / overall there, (mean / sqrt(overall))^2 here: a sqrt, two divisions and a product against a product
    # and a division, each rounding once
    again = B.link_apc(links[["pos1", "pos2", "MI"]], bg, snp)
    tol = 16 * 2.0 ** -53 * (np.abs(links["MI"].to_numpy()) + links["apc"].to_numpy())
    err = np.abs(links["mi_apc"].to_numpy() - again["mi_apc"].to_numpy())
    print("worst |mi_apc - link_apc| / tolerance:", float((err / tol).max()))
    assert (err <= tol).all() and np.array_equal(links["bg1"], again["bg1"]) and np.array_equal(links["bg2"], again["bg2"])
    idx = np.arange(120)
    M = engine.mi_block(idx, idx)                                              # the values the walk saw
    a, b = np.tril_indices(120, -1)
    order = np.argsort(-M[a, b], kind="stable")[:700]
    assert not ((a[order] == hi) & (b[order] == lo)).any()                     # a selection of the top 700 by raw MI does not hold the planted pair
    back = pd.read_csv(out, sep="\t", float_precision="round_trip")
    assert list(back.columns) == list(links.columns) and len(back) == 10
    for c in links.columns:
        assert np.allclose(links[c].to_numpy(dtype=np.float64), back[c].to_numpy(dtype=np.float64), rtol=1e-14, atol=0), c
    with pytest.raises(ValueError, match="which"):
        B.apc_links(snp, ones, which="long", engine=engine)
