"""GPU: ldw_mi_segment_map and ldw_mi_segment_best (Engine.mi_segment_map, Engine.mi_segment_best, ldweaver_amd.genemap; pytest -m gpu) on the
bundled sample alignment in blocks of 500 — against the numpy statement tests/segmap_ref.py applied to the engine's own dense blocks (exactly), against the
per-SNP summary and the pass's own pair counts, against the oracle's MI (n (MI_TIGHT + 2^-41) per cell) — and on the planted example through gene_map."""
import os

import numpy as np
import pandas as pd
import pytest

import caller_stream_job as J
import segmap_ref as G
import test_snpsum_gpu as SS
from ldweaver_amd import _lib as L
from ldweaver_amd import background as B
from ldweaver_amd import genemap as GM
from ldweaver_amd import mi as MIH
from ldweaver_amd import plots
from ldweaver_amd.cds import Annotation
from ldweaver_amd.engine import Engine
from ldweaver_amd.snpdat import SnpDat

pytestmark = pytest.mark.gpu

MI_TIGHT, SR_DIST, NSNP, QUIRKS = SS.MI_TIGHT, SS.SR_DIST, SS.NSNP, SS.QUIRKS
setup = SS.setup


@pytest.fixture(scope="module")
def prob(sample):
    return SS.Problem(sample)


def layouts(d, POS):
    """name -> (seg, S, class mask, weights or None): equal stretches of 7 and of 64, and an annotation with gaps and an overlap."""
    g = int(d["g"])
    rng = np.random.default_rng(4)
    starts = np.arange(1, g, g // 40)[:37]
    ends = starts + g // 60                                                     # gaps between the features ...
    ends[5] = starts[7] + 10                                                    # ... and one that overlaps its two successors
    ann = Annotation.from_arrays(starts, ends, "A" * g)
    from types import SimpleNamespace
    seg_a, table = GM.segments_from_annotation(SimpleNamespace(POS=POS), gff=ann)
    assert (seg_a < 0).any() and len(table) == 37 and not (seg_a == 6).any()
    return {"equal7": (GM.segments_equal(POS, g, 7), 7, 3, None), "equal64": (GM.segments_equal(POS, g, 64), 64, 2, rng.uniform(-0.2, 0.3, NSNP)),
            "annotation": (seg_a, 37, 1, None)}


def statement(prob, blocks_mi, POS, seg, S, mask, w, thr):
    tot = G.empty_map(S)
    for M, (fi, ti, diag) in zip(blocks_mi, prob.lists):
        G.add_block(tot, M, POS[fi], POS[ti], prob.d["g"], diag, seg[fi], seg[ti], SR_DIST, mask, None if w is None else w[fi], None if w is None else w[ti], thr)
    ref = G.finish(tot)
    best = np.full((S, S), G.NO_PAIR, dtype=np.uint64)
    for M, (fi, ti, diag) in zip(blocks_mi, prob.lists):
        G.best_block(best, ref["max"], M, POS[fi], POS[ti], prob.d["g"], diag, seg[fi], seg[ti], SR_DIST, mask, fi, ti, None if w is None else w[fi],
                     None if w is None else w[ti])
    return ref, best


@pytest.mark.parametrize("quirk", QUIRKS)
@pytest.mark.parametrize("order", ("ascending", "shuffled"))
def test_a_map_and_best_equal_the_statement_on_the_engines_own_blocks(engine, prob, quirk, order):
    POS = prob.d["POS"] if order == "ascending" else prob.shuffled
    setup(engine, prob.d, POS)
    thr = prob.thr(engine, quirk)[1]
    dense = prob.dense(engine, quirk)
    for name, (seg, S, mask, w) in layouts(prob.d, POS).items():
        ref, rbest = statement(prob, dense, POS, seg, S, mask, w, thr)
        got = engine.mi_segment_map(prob.blocks, seg, S, SR_DIST, mask, w, thr, quirk=quirk)
        for k in G.INTS:
            assert got[k].dtype == np.int64 and got[k].shape == (S, S) and np.array_equal(got[k], ref[k]), (name, k, np.argwhere(got[k] != ref[k])[:5])
        assert G.same_bits(got["max"], ref["max"]), name
        assert got["npairs"] == ref["npairs"] == int(got["n"].sum()) > 0 and ref["nge"].sum() > 0, name
        rep = engine.segment_map_report()
        assert rep["blocks"] == 6 and rep["patches"] > 0 and rep["refused"] == ref["refused"] == 0 and rep["nan_values"] == 0, (name, rep)
        if order == "ascending" and name == "equal7":
            assert rep["general"] == 0, (name, rep)                               # position-ordered SNPs in long segments: a few runs per patch
        t = engine.last_timing()
        assert t["gemm_ms"] > 0 and t["epilogue_ms"] > 0 and t["select_ms"] == 0 and abs(t["gemm_ms"] + t["epilogue_ms"] - t["total_ms"]) < 1e-6
        best = engine.mi_segment_best(prob.blocks, seg, S, SR_DIST, mask, got["max"], w, quirk=quirk)
        assert best.dtype == np.uint64 and np.array_equal(best, rbest), (name, np.argwhere(best != rbest)[:5])
        assert np.array_equal(best != G.NO_PAIR, ~np.isnan(got["max"]))
        assert engine.segment_map_report()["patches"] == rep["patches"] and engine.last_timing()["epilogue_ms"] > 0
    # the nullable outputs
    seg, S, mask, w = layouts(prob.d, POS)["equal7"]
    ref, _ = statement(prob, dense, POS, seg, S, mask, w, thr)
    import ctypes as C
    n, lo, hi, npairs = np.zeros((S, S), np.int64), np.zeros((S, S), np.int64), np.zeros((S, S), np.int64), C.c_int64(0)
    L.check(L.lib().ldw_mi_segment_map(engine._ctx, L.ptr(prob.blocks), 6, int(quirk), L.ptr(seg), S, SR_DIST, mask, None, thr, L.ptr(n), None, None, None, None, C.byref(npairs)))
    assert np.array_equal(n, ref["n"]) and npairs.value == ref["npairs"]
    L.check(L.lib().ldw_mi_segment_map(engine._ctx, L.ptr(prob.blocks), 6, int(quirk), L.ptr(seg), S, SR_DIST, mask, None, thr, L.ptr(n), None, L.ptr(lo), L.ptr(hi), None,
                                       C.byref(npairs)))
    assert np.array_equal(lo, ref["sum_lo"]) and np.array_equal(hi, ref["sum_hi"])
    assert L.lib().ldw_mi_segment_map(engine._ctx, L.ptr(prob.blocks), 6, int(quirk), L.ptr(seg), S, SR_DIST, mask, None, thr, L.ptr(n), None, L.ptr(lo), None, None,
                                      C.byref(npairs)) == L.LDW_ERR_ARG      # one sum word without the other


@pytest.mark.parametrize("order", ("ascending", "shuffled"))
def test_b_one_segment_per_snp_is_the_per_snp_summary(engine, prob, order):
    POS = prob.d["POS"] if order == "ascending" else prob.shuffled
    setup(engine, prob.d, POS)
    quirk = L.QUIRK_REFERENCE
    seg = np.arange(NSNP, dtype=np.int32)
    got = engine.mi_segment_map(prob.blocks, seg, NSNP, SR_DIST, 3, quirk=quirk)
    summ = engine.mi_snp_summary(prob.blocks, SR_DIST, quirk=quirk)
    assert not np.diag(got["n"]).any() and got["n"].max() == 1
    assert np.array_equal((got["n"] + got["n"].T).sum(axis=1), summ["n"].sum(axis=0))
    ex = G.exact(got)
    per_snp = (ex + ex.T).sum(axis=1)
    assert [int(x) for x in per_snp] == [int(x) for x in summ["sumq"].sum(axis=0)]      # bit for bit
    rep = engine.segment_map_report()
    assert rep["general"] == rep["patches"] > 0
    best = engine.mi_segment_best(prob.blocks, seg, NSNP, SR_DIST, 3, got["max"], quirk=quirk)
    r, c = np.nonzero(got["n"])
    assert np.array_equal(best[r, c], (r.astype(np.uint64) << np.uint64(32)) | c.astype(np.uint64)) and (best[got["n"] == 0] == G.NO_PAIR).all()
    for M, (fi, ti, diag) in zip(prob.dense(engine, quirk), prob.lists):      # every max is the dense value of the cell's own pair
        a, b = np.nonzero(G.pair_mask(len(fi), len(ti), diag))
        ga, gb = fi[a], ti[b]
        assert G.same_bits(got["max"][np.minimum(ga, gb), np.maximum(ga, gb)], M[a, b])


@pytest.mark.parametrize("quirk", QUIRKS)
def test_c_means_against_the_oracle(engine, prob, quirk):
    """Per cell |sum / 2^40 - sum of the oracle's MI| <= n (MI_TIGHT + 2^-41): MI_TIGHT bounds each value, 2^-41 is the half-unit of the fixed point
    (DESIGN.md 32's bound as it stands).  No cell is left out; the oracle's sum is taken in extended precision."""
    setup(engine, prob.d)
    POS = prob.d["POS"]
    seg = GM.segments_equal(POS, int(prob.d["g"]), 64)
    got = engine.mi_segment_map(prob.blocks, seg, 64, SR_DIST, 3, quirk=quirk)
    tot = np.zeros(64 * 64, dtype=np.longdouble)
    cnt = np.zeros(64 * 64, dtype=np.int64)
    for M, (fi, ti, diag) in zip(prob.oracle(quirk), prob.lists):
        m = G.pair_mask(len(fi), len(ti), diag)
        cell = G.cells(seg[fi], seg[ti], 64)[m]
        np.add.at(tot, cell, M[m].astype(np.longdouble))
        np.add.at(cnt, cell, 1)
    n = got["n"].reshape(-1)
    assert np.array_equal(cnt, n)
    ex = G.exact(got).reshape(-1)
    err = np.abs(np.array([np.longdouble(int(x)) for x in ex]) / np.longdouble(2.0 ** 40) - tot)      # (|sum| < 2^63 here: the integer converts exactly)
    bound = n * (MI_TIGHT + 2.0 ** -41)
    has = n > 0
    print("worst |sum - oracle| / bound:", float((err[has] / bound[has]).max()), "cells:", int(has.sum()))
    assert (err <= bound).all(), (np.flatnonzero(err > bound)[:5], err.max())
    gm = GM.GeneMap(got["n"], got["nge"], got["sum_lo"], got["sum_hi"], got["max"], None, got["npairs"], seg, POS, np.inf, "all", SR_DIST)
    mean_err = np.abs(gm.mean().reshape(-1)[has] - (tot[has] / n[has]).astype(np.float64))
    assert (mean_err <= MI_TIGHT + 2.0 ** -41 + 2.0 ** -52).all()               # (+ the rounding of the quotient itself)


@pytest.mark.parametrize("order", ("ascending", "shuffled"))
def test_d_the_pair_counts_are_the_passes_and_the_link_tables_stay(engine, prob, order):
    d = prob.d
    POS = d["POS"] if order == "ascending" else prob.shuffled
    setup(engine, d, POS)
    approx = MIH.lr_links_approx(POS, d["g"], SR_DIST)
    engine.reset_speculation()
    engine.mi_all_pairs(prob.blocks, SR_DIST, 2000.0, approx)
    stats = engine.block_stats()
    before = (engine.links_count(0), engine.links_count(1), engine.links(0), engine.links(1))
    seg = GM.segments_equal(POS, int(d["g"]), 7)
    n_sr, n_lr = int(stats["n_sr"].sum()), int(stats["n_lr_total"].sum())
    for mask, expect in ((1, n_sr), (2, n_lr), (3, n_sr + n_lr)):
        got = engine.mi_segment_map(prob.blocks, seg, 7, SR_DIST, mask)
        assert got["npairs"] == int(got["n"].sum()) == expect, (mask, got["npairs"], expect)
        assert not got["nge"].any()                                             # thr = +inf
        engine.mi_segment_best(prob.blocks, seg, 7, SR_DIST, mask, got["max"])
    after = (engine.links_count(0), engine.links_count(1), engine.links(0), engine.links(1))
    assert before[:2] == after[:2] and before[0] > 0 and before[1] > 0
    for tb, ta in zip(before[2:], after[2:]):
        for x, y in zip(tb, ta):
            assert np.array_equal(x, y)
    again = engine.block_stats()
    assert all(np.array_equal(stats[k], again[k]) for k in stats)


def test_e_on_a_caller_owned_stream_and_another_maps_maxima(engine, prob):
    setup(engine, prob.d)
    seg = GM.segments_equal(prob.d["POS"], int(prob.d["g"]), 64)
    ref = engine.mi_segment_map(prob.blocks, seg, 64, SR_DIST, 2, thr=0.05)
    rbest = engine.mi_segment_best(prob.blocks, seg, 64, SR_DIST, 2, ref["max"])
    with J.caller_stream("not_current") as cs:
        with Engine(0, stream=cs.handle) as eng:
            setup(eng, prob.d)
            got = eng.mi_segment_map(prob.blocks, seg, 64, SR_DIST, 2, thr=0.05)
            best = eng.mi_segment_best(prob.blocks, seg, 64, SR_DIST, 2, got["max"])
        assert cs.works()
    assert G.same_map(got, ref) and np.array_equal(best, rbest)
    # the second walk with the maxima of another threshold's map: the maxima do not depend on thr, so neither do the pairs
    other = engine.mi_segment_map(prob.blocks, seg, 64, SR_DIST, 2, thr=0.5)
    assert G.same_bits(other["max"], ref["max"]) and not np.array_equal(other["nge"], ref["nge"])
    assert np.array_equal(engine.mi_segment_best(prob.blocks, seg, 64, SR_DIST, 2, other["max"]), rbest)
    # maxima of another class name nothing where no pair of this class has those bits; NaN names nothing
    sr_max = engine.mi_segment_map(prob.blocks, seg, 64, SR_DIST, 1)["max"]
    cross = engine.mi_segment_best(prob.blocks, seg, 64, SR_DIST, 2, sr_max)
    dense = prob.dense(engine, L.QUIRK_REFERENCE)
    _, expect = None, np.full((64, 64), G.NO_PAIR, dtype=np.uint64)
    for M, (fi, ti, diag) in zip(dense, prob.lists):
        G.best_block(expect, sr_max, M, prob.d["POS"][fi], prob.d["POS"][ti], prob.d["g"], diag, seg[fi], seg[ti], SR_DIST, 2, fi, ti)
    assert np.array_equal(cross, expect)
    assert (engine.mi_segment_best(prob.blocks, seg, 64, SR_DIST, 2, np.full((64, 64), np.nan)) == G.NO_PAIR).all()


def test_states_and_refusals(engine, prob):
    seg = np.zeros(NSNP, dtype=np.int32)
    with Engine(0) as eng:
        with pytest.raises(L.LdwError) as e:                                    # nothing set
            eng.mi_segment_map(prob.blocks, seg, 1, SR_DIST, 3)
        assert e.value.code == L.LDW_ERR_STATE and "ldw_mi_segment_map" in str(e.value)
    setup(engine, prob.d)
    for bad in ([1, 500, 400, 900], [1, 500, 1, 400], [0, 500, 0, 500], [1, 1269, 1, 1269]):
        with pytest.raises(L.LdwError) as e:
            engine.mi_segment_map(np.array([bad], dtype=np.int32), seg, 1, SR_DIST, 3)
        assert e.value.code == L.LDW_ERR_ARG and "ldw_mi_segment_map" in str(e.value), bad
        with pytest.raises(L.LdwError) as e:
            engine.mi_segment_best(np.array([bad], dtype=np.int32), seg, 1, SR_DIST, 3, np.zeros((1, 1)))
        assert e.value.code == L.LDW_ERR_ARG and "ldw_mi_segment_best" in str(e.value), bad
    w_bad = np.zeros(NSNP)
    w_bad[17] = np.inf
    seg_bad = seg.copy()
    seg_bad[[40, 90]] = 3, -2
    for kw, match in ((dict(S=0), "S 0"), (dict(S=8193), "S 8193"), (dict(seg=seg_bad, S=3), "seg[40]"), (dict(sr_dist=-1.0), "sr_dist"), (dict(sr_dist=np.nan), "sr_dist"),
                      (dict(cls_mask=0), "cls_mask"), (dict(cls_mask=4), "cls_mask"), (dict(w=w_bad), "w[17]")):
        a = dict(blocks=prob.blocks, seg=seg, S=1, sr_dist=SR_DIST, cls_mask=3, w=None)
        a.update(kw)
        with pytest.raises(L.LdwError) as e:
            engine.mi_segment_map(**a)
        assert e.value.code == L.LDW_ERR_ARG and match in str(e.value), (kw, str(e.value))
        with pytest.raises(L.LdwError) as e:
            engine.mi_segment_best(max_in=np.zeros((1, 1)) if not 1 < a["S"] <= 8192 else np.zeros((a["S"], a["S"])), **a)
        assert e.value.code == L.LDW_ERR_ARG and match in str(e.value), (kw, str(e.value))
    got = engine.mi_segment_map(np.array([[501, 1000, 1, 500]], dtype=np.int32), np.where(np.arange(NSNP) < 500, 1, 0).astype(np.int32), 2, np.inf, 1)
    assert got["n"].tolist() == [[0, 500 * 500 - 500], [0, 0]] and got["npairs"] == 500 * 500 - 500      # disjoint, the to side first; the from-segment below the to-segment


def test_the_planted_example_through_gene_map(engine, tmp_path):
    """By raw nge the marker segments' cells rank first; with the average product correction (background=) the planted cell ranks first and its best pair
    is a planted pair.  tests/test_segmap_host.py checks the same claims on the C oracle's values."""
    st, pos, g, sr, seg, marker_segs, cell, pairs = G.planted_genes()
    snp = SnpDat.from_states(st, pos, g)
    ones = np.ones(st.shape[1])
    thr = 0.2
    out, png = tmp_path / "genemap.tsv", tmp_path / "genemap.png"
    raw = GM.gene_map(snp, ones, segments=seg, sr_dist=sr, which="lr", thr=thr, engine=engine, out_path=str(out), plot_path=str(png))
    assert raw.S == 12 and raw.npairs == 120 * 119 // 2 and raw.pair is not None
    fr = raw.frame()
    marker_cells = {(a, b) for a in marker_segs for b in marker_segs if a < b}
    assert {(int(a), int(b)) for a, b in fr[["seg1", "seg2"]].values[:6]} == marker_cells and (fr["nge"][:6] == 100).all() and (fr["n"] == 100).all()
    assert tuple(fr[["seg1", "seg2"]].values[6]) == cell and fr["nge"][6] == 5
    bg = B.snp_background(snp, ones, sr_dist=sr, engine=engine)
    apc = GM.gene_map(snp, ones, segments=seg, n_segments=12, sr_dist=sr, which="lr", thr=thr, background=bg, engine=engine, alignment_resident=True)
    fa = apc.frame()
    print("corrected: planted nge", fa["nge"][0], "max", fa["max"][0], "next nge", fa["nge"][1], "largest marker max", max(apc.max[c] for c in marker_cells))
    assert tuple(fa[["seg1", "seg2"]].values[0]) == cell and fa["nge"][0] == 5 and fa["nge"][1] == 0
    assert max(apc.max[c] for c in marker_cells) < 0.5 * thr
    p = int(apc.pair[cell])
    assert (p >> 32, p & 0xFFFFFFFF) in pairs and (fa["pos1"][0], fa["pos2"][0]) == (float(pos[p >> 32]), float(pos[p & 0xFFFFFFFF]))
    idx = np.arange(len(st))
    M = engine.mi_block(idx, idx)                                              # the values the map saw: the engine still holds the problem
    w = B.apc_weights(bg, "lr")
    ref = G.segment_map(M, pos, pos, g, True, seg, seg, 12, sr, 2, w, w, thr)
    assert all(np.array_equal(getattr(apc, k), ref[k]) for k in G.INTS) and G.same_bits(apc.max, ref["max"])
    assert np.array_equal(apc.pair, G.segment_best(M, pos, pos, g, True, seg, seg, 12, sr, 2, idx, idx, ref["max"], w, w))
    with pytest.raises(ValueError):
        GM.gene_map(snp, ones, segments=seg, w=w, background=bg, engine=engine)
    nobest = GM.gene_map(snp, ones, segments=seg, sr_dist=sr, which="all", best=False, engine=engine)
    assert nobest.pair is None and np.isnan(nobest.frame()["pos1"]).all() and nobest.npairs == raw.npairs and not nobest.nge.any()
    full = raw.frame(include_diagonal=True)
    back = pd.read_csv(out, sep="\t", float_precision="round_trip")
    assert list(back.columns) == list(full.columns) and len(back) == len(full) == 78
    for c in full.columns:      # the native writer prints R's 15 significant digits: equal to that precision, integers exactly
        x, y = full[c].to_numpy(dtype=np.float64), back[c].to_numpy(dtype=np.float64)
        assert np.array_equal(np.isnan(x), np.isnan(y)) and np.allclose(x[~np.isnan(x)], y[~np.isnan(y)], rtol=1e-14, atol=0), c
    with open(png, "rb") as f:
        head = f.read(24)
    assert head[:8] == b"\x89PNG\r\n\x1a\n" and os.path.getsize(png) > 1000
    for by in plots.GENE_MAP_BY:
        plots.gene_map_plot(apc, str(tmp_path / f"{by}.png"), by, engine=engine)
        assert os.path.getsize(tmp_path / f"{by}.png") > 1000
