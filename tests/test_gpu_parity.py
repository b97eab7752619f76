"""GPU parity tests (pytest -m gpu): the HIP path, called through the C ABI, against the CPU oracle on the same
inputs, against the committed golden fixtures, and — at BASELINE.json's sizes — through size-independent properties.
Bars: integer / index work bit-exact; MI within 1e-6 (north_star), typically ~1e-12 (weight quantisation)."""
import json
import os
import sys

import numpy as np
import pandas as pd
import pytest

import c_oracle
import ldw_oracle as orc
from ldweaver_amd import _lib as L
from ldweaver_amd import mi as MIH
from ldweaver_amd import srp as srp_host
from ldweaver_amd.engine import Engine
from ldweaver_amd.snpdat import CdsVar, SnpDat
from ldweaver_amd.synth import synth_alignment

pytestmark = pytest.mark.gpu
MI_TOL = 1e-6          # tolerance stated by BASELINE.json's north_star
MI_TIGHT = 1e-10       # what the 40-bit fixed-point weights actually deliver


def _setup(eng, d, nlimbs=0):
    eng.set_engine(L.ENGINE_MFMA)
    eng.set_alignment(d["states"])
    eng.set_weights(d["hdw"], nlimbs)
    eng.set_snp_meta(d["r"], d["uqe"], d["POS"], d["paint"], d["g"])


def test_alignment_roundtrip_counts_and_encoder(engine, sample):
    st = sample["states"]
    engine.set_alignment(st)
    assert np.array_equal(engine.get_alignment(), st)
    assert np.array_equal(engine.state_counts(), orc.acgtn_table(st))
    # device encoder (src/getACGTNsites.cpp:229-265): mixed case, IUPAC, gaps; retained-column gather
    rng = np.random.default_rng(0)
    chars = rng.choice(np.frombuffer(b"ACGTacgtNn-RYK*", dtype=np.uint8), size=(37, 501))
    pos = np.sort(rng.choice(501, 133, replace=False) + 1).astype(np.int32)
    tab = engine.encode_alignment(chars, pos)
    ref = orc.encode_states([bytes(row[pos - 1]) for row in chars])
    assert np.array_equal(engine.get_alignment(), ref)
    assert np.array_equal(tab, orc.acgtn_table(ref))


def test_hamming_weights_bit_exact(engine, sample, synth):
    for d, thr in ((sample, 0.1), (synth, 0.1), (synth, 0.25)):
        st = d["states"]
        engine.set_alignment(st)
        thresh = int(st.shape[0] * thr)
        hdw, shared = engine.hamming_weights(thresh, want_shared=True)
        assert np.array_equal(shared, orc.shared_counts(st))
        assert np.array_equal(hdw, orc.hamming_weights(st, thr))
    assert np.array_equal(engine.hamming_weights(int(512 * 0.1)), synth["hdw"])      # golden
    # threshold 0: nobody is closer than 0 mismatches -> all weights 1; huge threshold -> 1/(N+1)
    engine.set_alignment(sample["states"])
    assert np.array_equal(engine.hamming_weights(0), np.ones(400))
    assert np.array_equal(engine.hamming_weights(10 ** 6), np.full(400, 1 / 401))


def test_joint_counts_bit_exact(engine, sample, synth):
    for d in (sample, synth):
        _setup(engine, d)
        st = d["states"]
        rng = np.random.default_rng(2)
        pa, pb = rng.integers(0, st.shape[0], 400), rng.integers(0, st.shape[0], 400)
        pa[:4], pb[:4] = (0, 5, st.shape[0] - 1, 100), (1, 300, 17, 100)       # includes a self pair
        cnt, fix, fb = engine.joint_tables(pa, pb)
        sq = np.sqrt(d["hdw"])
        V = np.rint(np.ldexp(sq * sq, fb)).astype(np.int64)
        for k in range(len(pa)):
            code = st[pa[k]].astype(np.int64) * 5 + st[pb[k]]
            assert np.array_equal(cnt[k], np.bincount(code, minlength=25).reshape(5, 5))
            assert np.array_equal(fix[k].ravel(), np.array([V[code == c].sum() for c in range(25)]))
    assert np.array_equal(cnt[:4], synth["joint_counts"])                       # golden


@pytest.mark.parametrize("eng_kind", [L.ENGINE_MFMA, L.ENGINE_HIST])
def test_mi_blocks_match_oracle_and_golden(engine, sample, eng_kind):
    _setup(engine, sample)
    engine.set_engine(eng_kind)
    idx = np.arange(1268)
    MI = engine.mi_block(idx, idx)
    assert np.abs(MI[np.ix_(sample["sub_r"], sample["sub_c"])] - sample["MI_single_sub"]).max() < MI_TIGHT
    assert np.abs(MI.sum(axis=0) - sample["MI_single_colsum"]).max() < 1e-7
    st = sample["states"]
    for bi, (fs, fe, ts, te) in enumerate(sample["blocks"]):   # forced multi-block: Q1 on the non-square block
        fi, ti = np.arange(fs - 1, fe), np.arange(ts - 1, te)
        Mb = engine.mi_block(fi, ti)
        ref = c_oracle.mi_block(st, sample["hdw"], sample["r"], sample["uqe"], fi, ti)
        assert np.abs(Mb - ref).max() < MI_TIGHT
        assert np.abs(Mb[::7, ::5] - sample[f"MI_blk{bi}_sub"]).max() < MI_TIGHT
    engine.set_engine(L.ENGINE_MFMA)


def test_quirk_modes(engine, sample):
    _setup(engine, sample)
    fs, fe, ts, te = sample["blocks"][1]
    fi, ti = np.arange(fs - 1, fe), np.arange(ts - 1, te)
    Mq = engine.mi_block(fi, ti, quirk=L.QUIRK_REFERENCE)
    Mi = engine.mi_block(fi, ti, quirk=L.QUIRK_INTENDED)
    assert np.abs(Mq - Mi).max() > 1e-4                      # the scramble is visible on a non-square block
    st, hdw, r, uqe = sample["states"], sample["hdw"], sample["r"], sample["uqe"]
    for a, b in ((0, 0), (999, 267), (17, 133)):
        assert abs(Mi[a, b] - orc.mi_pair_direct(st, hdw, r, uqe, fi[a], ti[b])) < MI_TIGHT
        assert abs(Mq[a, b] - orc.mi_pair_direct(st, hdw, r, uqe, fi[a], ti[b], orc.q1_rxy(a, b, 1000, 268, r[fi], r[ti]))) < MI_TIGHT
    # intended mode is symmetric under exchanging the two sides
    Mt = engine.mi_block(ti, fi, quirk=L.QUIRK_INTENDED)
    assert np.abs(Mi - Mt.T).max() < 1e-12


@pytest.mark.parametrize("nlimbs,tol", [(3, 1e-4), (4, 1e-7), (5, 1e-10), (6, 1e-12)])
def test_limb_precision_ladder(engine, synth, nlimbs, tol):
    _setup(engine, synth, nlimbs)
    idx = np.arange(512)
    MI = engine.mi_block(idx, idx)
    err = np.abs(MI[::3, ::5] - synth["MI_sub"]).max()
    assert err < tol, err
    assert np.abs(MI.sum(axis=1) - synth["MI_rowsum"]).max() < tol * 512


def test_unit_weights_are_exact_counts(engine, synth):
    d = dict(synth)
    d["hdw"] = np.ones(1000)
    _setup(engine, d, 1)
    cnt, fix, fb = engine.joint_tables([3, 400], [77, 2])
    assert fb == 0 and np.array_equal(cnt, fix)
    idx = np.arange(128)
    MI = engine.mi_block(idx, idx)
    ref = c_oracle.mi_block(d["states"], d["hdw"], d["r"], d["uqe"], idx, idx)
    assert np.abs(MI - ref).max() < 1e-12


def test_edge_cases_ragged_and_degenerate(engine):
    """N not a multiple of the K step, tiny blocks, a monomorphic column, an all-gap column, a 5-state column,
    uqe that disagrees with the data (flag set for an absent state / cleared for a present one)."""
    rng = np.random.default_rng(11)
    Ls, Ns = 77, 131
    st = rng.integers(0, 2, (Ls, Ns)).astype(np.uint8)
    st[3] = 2                              # monomorphic
    st[4] = 4                              # all gaps
    st[5] = rng.integers(0, 5, Ns)         # all five states
    st[6, :5] = (0, 1, 2, 3, 4)
    uqe, r = orc.uqe_r(st)
    uqe[7, 3] = 1.0                        # flagged but absent
    uqe[8, 0] = 0.0                        # present but masked
    hdw = rng.choice([1.0, 0.5, 1 / 3, 1 / 7, 1 / 131], Ns)
    POS = np.sort(rng.choice(5000, Ls, replace=False) + 1).astype(np.int32)
    d = dict(states=st, hdw=hdw, r=r, uqe=uqe, POS=POS, paint=np.ones(Ls, dtype=np.int32), g=5001.0)
    for kind in (L.ENGINE_MFMA, L.ENGINE_HIST):
        _setup(engine, d)
        engine.set_engine(kind)
        for fi, ti in ((np.arange(Ls), np.arange(Ls)), (np.arange(0, 40), np.arange(40, 77)), (np.array([5]), np.array([6])),
                       (np.array([3, 4, 5, 7, 8]), np.arange(Ls))):
            MI = engine.mi_block(fi, ti)
            ref = c_oracle.mi_block(st, hdw, r, uqe, fi, ti)
            assert np.abs(MI - ref).max() < MI_TIGHT, (kind, len(fi), len(ti))
    engine.set_engine(L.ENGINE_MFMA)
    with pytest.raises(L.LdwError):
        engine.mi_block(np.array([Ls]), np.array([0]))           # index out of range
    with pytest.raises(L.LdwError):
        engine.mi_block(np.array([], dtype=np.int32), np.array([0]))  # empty block
    with pytest.raises(L.LdwError):
        engine.set_weights(np.ones(Ns + 1))                      # wrong length
    with pytest.raises(L.LdwError):
        engine.set_weights(np.full(Ns, -1.0))


def _check_tables(eng, d, tag, POS, paint):
    a, b, mi = eng.links(1)
    assert len(mi) == int(d[f"{tag}_lr_n"])
    pos1, pos2 = POS[b].astype(float), POS[a].astype(float)
    assert np.array_equal(pos1[:200], d[f"{tag}_lr_pos1_head"]) and np.array_equal(pos2[-200:], d[f"{tag}_lr_pos2_tail"])
    assert np.abs(mi[:200] - d[f"{tag}_lr_MI_head"]).max() < MI_TIGHT and np.abs(mi[-200:] - d[f"{tag}_lr_MI_tail"]).max() < MI_TIGHT
    w = np.arange(len(mi)) % 1009 + 1
    assert abs((pos1 * w).sum() - float(d[f"{tag}_lr_pos1_wsum"])) < 1e-3      # order-sensitive checksum of the whole table
    a, b, mi = eng.links(0)
    pos1, pos2, c1, c2 = POS[b].astype(float), POS[a].astype(float), paint[b], paint[a]
    for ci in (1, 2, 3):
        sel = (c1 == ci) | (c2 == ci)
        n = int(sel.sum())
        assert n == int(d[f"{tag}_sr{ci}_n"])
        assert np.array_equal(pos1[sel][:200], d[f"{tag}_sr{ci}_pos1_head"]) and np.array_equal(pos2[sel][-200:], d[f"{tag}_sr{ci}_pos2_tail"])
        w = np.arange(n) % 1009 + 1
        assert abs((pos2[sel] * w).sum() - float(d[f"{tag}_sr{ci}_pos2_wsum"])) < 1e-3
        assert abs((mi[sel] * w).sum() - float(d[f"{tag}_sr{ci}_MI_wsum"])) < MI_TIGHT * w.sum()  # mean |dMI| below 1e-10


def test_link_tables_match_golden(engine, sample):
    """The a-5 loop: row counts, row ORDER (Q3/Q4) and values of the sr / lr tables, single- and multi-block."""
    _setup(engine, sample)
    for tag, mb, retain in (("single", 10000, 1e6), ("multi", 1000, 1e5)):
        blocks = MIH.make_blocks(1268, mb)
        engine.mi_all_pairs(blocks, 20000.0, retain, float(sample[f"{tag}_lr_approx"]))
        _check_tables(engine, sample, tag, sample["POS"], sample["paint"])
        for which in (0, 1):     # the zero-copy device view (ldw_links_device_ptrs) shows the same table
            for x, y in zip(engine.links(which), engine.links_view(which)):
                assert y.is_cuda and np.array_equal(x, y.cpu().numpy())
        st = engine.block_stats()
        assert st["n_lr_kept"].sum() == int(sample[f"{tag}_lr_n"])


def test_lr_quantile_filter_exact(engine, synth):
    """Per-block type-7 quantile threshold and retained set == oracle when only a small top fraction is kept."""
    _setup(engine, synth)
    POS, g = synth["POS"], synth["g"]
    approx = orc.lr_links_approx(POS, g, 20000.0)
    for retain, mb in ((500.0, 10000), (2000.0, 1000)):
        blocks = orc.make_blocks(512, orc.r_round_thousands(mb))
        engine.mi_all_pairs(np.array(blocks, dtype=np.int32), 20000.0, retain, approx)
        st = engine.block_stats()
        a, b, mi = engine.links(1)
        off = 0
        for bi, (fs, fe, ts, te) in enumerate(blocks):
            fi, ti = np.arange(fs - 1, fe), np.arange(ts - 1, te)
            Mb = c_oracle.mi_block(synth["states"], synth["hdw"], synth["r"], synth["uqe"], fi, ti)
            bl = orc.block_links(Mb, fi, ti, POS, synth["paint"], g, 20000.0, retain, approx)
            assert st["n_lr_total"][bi] == bl.n_lr_total
            n = len(bl.lr["MI"])
            assert st["n_lr_kept"][bi] == n, (bi, st["n_lr_kept"][bi], n)
            assert abs(st["disc_thresh"][bi] - bl.disc_thresh) < MI_TIGHT
            assert np.array_equal(a[off:off + n], bl.lr["a"]) and np.array_equal(b[off:off + n], bl.lr["b"])
            assert np.abs(mi[off:off + n] - bl.lr["MI"]).max() < MI_TIGHT
            off += n
        assert off == len(mi)


@pytest.mark.parametrize("variant", ["default", "plain", "limb_paths", "sort_select"])
def test_threshold_ties_match_oracle_exactly(engine, sample, variant):
    """Ties at a block's long-range threshold (R/computePairwiseMI.R:352-358: `MI >= quantile(MI, prob)`): the reference's
    sample alignment is clonal — a third of its links sit in groups of pairs with identical joint tables, and several blocks'
    thresholds fall INSIDE such a group.  The reference keeps or drops a group as one (bitwise-equal MI, `>=`); so must we:
    the emitted fp64 MI is a pure function of the slot-ordered joint table (same cell order and arithmetic in every kernel
    variant), hence the retained (a, b) set of every block equals the oracle's EXACTLY — no tolerance for threshold ties —
    on every execution path, cold and warm."""
    _setup(engine, sample)
    POS, g = sample["POS"], sample["g"]
    approx = orc.lr_links_approx(POS, g, 20000.0)
    blocks = np.array(orc.make_blocks(1268, 300), dtype=np.int32)      # 5 x 5 grid, 15 block pairs, ragged last column
    cfg = dict(default=(True, 1, 0), plain=(False, 0, 1), limb_paths=(True, 1, 1), sort_select=(True, 1, 0))[variant]
    engine.set_select(1 if variant == "sort_select" else 0)     # the general selection path (two radix sorts) against the sort-free one
    engine.set_mixed(cfg[0])
    engine.set_screen(cfg[1])
    engine.set_path(cfg[2])
    try:
        runs = []
        for _ in range(2):      # cold (no bucket guesses), then warm (speculative blocks: screen / approximate paths)
            engine.mi_all_pairs(blocks, 20000.0, 40000.0, approx)
            runs.append((engine.links(1), engine.block_stats()))
    finally:
        engine.set_mixed(True)
        engine.set_screen(1)
        engine.set_path(0)
        engine.set_select(0)
    tied_blocks = 0
    for (a, b, mi), st in runs:
        off = 0
        for bi, (fs, fe, ts, te) in enumerate(blocks.tolist()):
            fi, ti = np.arange(fs - 1, fe), np.arange(ts - 1, te)
            Mb = c_oracle.mi_block(sample["states"], sample["hdw"], sample["r"], sample["uqe"], fi, ti)
            bl = orc.block_links(Mb, fi, ti, POS, sample["paint"], g, 20000.0, 40000.0, approx)
            n = len(bl.lr["MI"])
            assert st["n_lr_kept"][bi] == n, (variant, bi, int(st["n_lr_kept"][bi]), n)
            assert np.array_equal(a[off:off + n], bl.lr["a"]) and np.array_equal(b[off:off + n], bl.lr["b"]), (variant, bi)
            if n and (bl.lr["MI"] == bl.lr["MI"].min()).sum() > 1 and (Mb == bl.lr["MI"].min()).sum() > 1:
                tied_blocks += 1       # the smallest kept value is shared by several pairs: a tie group sits on the threshold
                # (our groups can only be coarser than the reference's: equal slot-ordered tables give equal bits here, while the
                # reference's fixed A,C,G,T,N summation order separates relabelled copies in the last bit)
                assert (mi[off:off + n] == mi[off:off + n].min()).sum() >= (bl.lr["MI"] == bl.lr["MI"].min()).sum()
            off += n
        assert off == len(mi)
    assert tied_blocks >= 4, tied_blocks


def test_perform_mi_computation_end_to_end(engine, sample, tmp_path):
    """Drop-in entry point with the reference's signature: returned frame and both tsv files vs the oracle's a-5 loop
    (srp model: same optimiser on both sides; parity with R's fitdist is unpinned)."""
    st = sample["states"]
    sd = SnpDat(states=st, POS=sample["POS"], g=sample["g"], uqe=sample["uqe"], r=sample["r"])
    cv = CdsVar(paint=sample["paint"], nclust=3)
    lr_p, sr_p = str(tmp_path / "lr.tsv"), str(tmp_path / "sr.tsv")
    red, aux = MIH.perform_MI_computation(sd, sample["hdw"], cv, ncores=1, lr_save_path=lr_p, sr_save_path=sr_p,
                                          plt_folder=str(tmp_path / "plots"), max_blk_sz=10000, lr_retain_links=1e6,
                                          engine=engine, verbose=False, return_aux=True)
    ref = orc.perform_mi_computation(st, sample["POS"], sample["g"], sample["r"], sample["uqe"], sample["hdw"], sample["paint"], 3,
                                     lr_retain_links=1e6, max_blk_sz=10000)
    rr = ref.sr_links_red
    assert len(red) == len(rr["MI"]) > 100
    # both are ordered by decreasing srp_max; MI differs by ~1e-12 so near-ties may swap: compare as keyed tables
    assert (np.diff(red["srp_max"].to_numpy()) <= 0).all()
    ko = np.lexsort((np.asarray(rr["clust_c"]), rr["pos2"], rr["pos1"]))
    kg = np.lexsort((red["clust_c"].to_numpy(), red["pos2"].to_numpy(), red["pos1"].to_numpy()))
    for k in ("clust_c", "pos1", "pos2", "clust1", "clust2", "len"):
        assert np.array_equal(red[k].to_numpy(dtype=float)[kg], np.asarray(rr[k], dtype=float)[ko]), k
    # ARACNE is a chain of strict MI comparisons: exact on identical inputs; against the oracle's own MI (1e-12 away)
    # only exact MI ties (SNPs in perfect LD) may flip
    chk = aux["sr_links_ARACNE_check"]
    flags = orc.run_aracne(red["pos1"].to_numpy(), red["pos2"].to_numpy(), red["MI"].to_numpy(), chk["pos1"].to_numpy(),
                           chk["pos2"].to_numpy(), chk["MI"].to_numpy())
    assert np.array_equal(red["ARACNE"].to_numpy(), flags.astype(float))
    # links whose triangle test is decided by a margin > eps must agree with the oracle's flags; the rest are exact ties
    eps = 1e-9
    adj = {}
    for p1, p2, m in zip(chk["pos1"].to_numpy(), chk["pos2"].to_numpy(), chk["MI"].to_numpy()):
        adj.setdefault(p1, {}).setdefault(p2, m)
        adj.setdefault(p2, {}).setdefault(p1, m)
    got, want = red["ARACNE"].to_numpy()[kg], np.asarray(rr["ARACNE"])[ko]
    n_decided = 0
    for i, (x, z, m0) in enumerate(zip(red["pos1"].to_numpy()[kg], red["pos2"].to_numpy()[kg], red["MI"].to_numpy()[kg])):
        common = set(adj.get(x, {})) & set(adj.get(z, {}))
        surely_indirect = any(m0 < adj[x][y] - eps and m0 < adj[z][y] - eps for y in common)
        maybe_indirect = any(m0 < adj[x][y] + eps and m0 < adj[z][y] + eps for y in common)
        if surely_indirect or not maybe_indirect:
            n_decided += 1
            assert got[i] == want[i] == (0.0 if surely_indirect else 1.0), (i, x, z)
    assert n_decided > 0.5 * len(got)   # the sample is clonal: ~1/3 of its links sit in exact MI ties (perfect LD)
    assert np.abs(red["MI"].to_numpy()[kg] - rr["MI"][ko]).max() < MI_TIGHT
    assert np.abs(red["srp_max"].to_numpy()[kg] - rr["srp_max"][ko]).max() < 1e-6
    assert 0 < red["ARACNE"].sum() < len(red)
    lines = open(lr_p).read().splitlines()
    assert len(lines) == len(ref.lr_rows["MI"]) == int(sample["single_lr_n"])
    first = lines[0].split("\t")
    assert len(first) == 6 and float(first[0]) == ref.lr_rows["pos1"][0] and abs(float(first[5]) - ref.lr_rows["MI"][0]) < 1e-9
    srl = open(sr_p).read().splitlines()
    assert len(srl) == len(red) and len(srl[0].split("\t")) == 9
    # the maxvls table the reference saves as c<i>_fit_data.rds (len, 95th percentile of MI at that len, fitted decay; :422-439)
    assert len(aux["fit_data"]) == len(ref.fit_data) == 3
    for ci, (fd, ofd) in enumerate(zip(aux["fit_data"], ref.fit_data)):
        assert np.array_equal(fd["len"].to_numpy(), ofd["len"]) and len(fd) > 100
        assert np.abs(fd["max"].to_numpy() - ofd["max"]).max() < MI_TIGHT
        assert np.abs(fd["fit"].to_numpy() / ofd["fit"] - 1).max() < 1e-8
        tsv = pd.read_csv(tmp_path / "plots" / f"c{ci + 1}_fit_data.tsv", sep="\t")
        assert list(tsv.columns) == ["len", "max", "fit"] and len(tsv) == len(fd)


def test_links_tsv_written_beside_other_calls(engine, synth, tmp_path):
    """ldw_write_links_tsv_begin / _end: the table is fetched at _begin, so the file holds THAT table byte for byte whatever the context does
    before _end (here: the short-range reductions, and a replacement of the table itself); a second _begin finishes the first; _end without
    _begin reports nothing; an unwritable path is reported by _end."""
    d = synth
    _setup(engine, d)
    engine.mi_all_pairs(orc.make_blocks(512, 1000), sr_dist=3000.0, lr_retain_links=1e6, lr_links_approx=1e5)
    for which in (1, 0):
        sync_p, async_p = tmp_path / f"sync{which}.tsv", tmp_path / f"async{which}.tsv"
        rows, nbytes = engine.write_links_tsv(which, str(sync_p), append=False)
        a, b, mi = engine.links(which)
        engine.write_links_tsv_begin(which, str(async_p), append=False)
        engine.sr_len_quantiles(3, 3000.0, 0.95)                      # GPU work of the same context meanwhile
        engine.links_import(which, a[::-1].copy(), b[::-1].copy(), mi[::-1].copy())   # ... and the table itself replaced
        assert engine.write_links_tsv_end() == (rows, nbytes)
        assert async_p.read_bytes() == sync_p.read_bytes() and rows == len(mi) > 0
        engine.links_import(which, a, b, mi)
    assert engine.write_links_tsv_end() == (0, 0)
    engine.write_links_tsv_begin(1, str(tmp_path / "first.tsv"), append=False)
    engine.write_links_tsv_begin(1, str(tmp_path / "second.tsv"), append=False)     # finishes "first"
    assert (tmp_path / "first.tsv").read_bytes() == (tmp_path / "sync1.tsv").read_bytes()
    engine.write_links_tsv_end()
    assert (tmp_path / "second.tsv").read_bytes() == (tmp_path / "sync1.tsv").read_bytes()
    # append mode continues an existing file
    (tmp_path / "app.tsv").write_text("header\n")
    engine.write_links_tsv_begin(1, str(tmp_path / "app.tsv"), append=True)
    engine.write_links_tsv_end()
    assert (tmp_path / "app.tsv").read_bytes() == b"header\n" + (tmp_path / "sync1.tsv").read_bytes()
    with pytest.raises(RuntimeError):
        engine.write_links_tsv_begin(1, str(tmp_path / "no_such_dir" / "x.tsv"), append=False)
        engine.write_links_tsv_end()


@pytest.mark.parametrize("max_blk_sz", [10000, 1000])
def test_device_sr_model_matches_host_model(engine, sample, tmp_path, max_blk_sz):
    """mergeNsort_sr_links + runARACNE on the device-resident link table (csrc/ldw_srp.hip) against the host mirror
    (pandas + the native ARACNE) on the same MI table: same rows in the same order, srp within 1e-9, same flags; against
    the oracle's model and ARACNE on that table; and each device reduction against numpy on the fetched table."""
    st = sample["states"]
    sd = SnpDat(states=st, POS=sample["POS"], g=sample["g"], uqe=sample["uqe"], r=sample["r"])
    cv = CdsVar(paint=sample["paint"], nclust=3)
    kw = dict(ncores=1, plt_folder=str(tmp_path / "plots"), max_blk_sz=max_blk_sz, lr_retain_links=1e6, engine=engine,
              verbose=False, return_aux=True, order_links=False, srp_cutoff=2.0,
              quirk_mode=L.QUIRK_REFERENCE if max_blk_sz == 10000 else L.QUIRK_INTENDED)
    out = {}
    for model in ("host", "device"):
        out[model] = MIH.perform_MI_computation(sd, sample["hdw"], cv, lr_save_path=str(tmp_path / f"lr_{model}.tsv"),
                                                sr_save_path=str(tmp_path / f"sr_{model}.tsv"), sr_model=model, **kw)
    (rh, ah), (rd, ad) = out["host"], out["device"]
    assert len(rh) == len(rd) > 100
    for k in ("clust_c", "pos1", "pos2", "clust1", "clust2", "len", "MI", "ARACNE"):
        assert np.array_equal(rh[k].to_numpy(dtype=float), rd[k].to_numpy(dtype=float)), k
    np.testing.assert_allclose(rd["srp_max"].to_numpy(), rh["srp_max"].to_numpy(), rtol=1e-9)
    assert 0 < rd["ARACNE"].sum() < len(rd) and (rd["clust1"] != rd["clust2"]).any()
    ch, cd = ah["sr_links_ARACNE_check"], ad["sr_links_ARACNE_check"]
    key = lambda f: np.lexsort((f["pos2"].to_numpy(), f["pos1"].to_numpy()))
    assert len(ch) == len(cd)
    for k in ("pos1", "pos2", "MI"):
        assert np.array_equal(ch[k].to_numpy()[key(ch)], cd[k].to_numpy()[key(cd)]), k
    hl, dl = open(tmp_path / "sr_host.tsv").read().splitlines(), open(tmp_path / "sr_device.tsv").read().splitlines()
    assert len(hl) == len(dl) == len(rd)
    for x, y in zip(hl, dl):   # identical text except the 15-digit srp_max column
        x, y = x.split("\t"), y.split("\t")
        assert x[:7] == y[:7] and x[8] == y[8] and abs(float(x[7]) - float(y[7])) <= 1e-9 * float(x[7])

    # the reductions one by one, on the table the engine still holds
    a, b, mi = engine.links(0)
    POS, paint, g = sample["POS"].astype(float), sample["paint"], float(sample["g"])
    ln = orc.circ_len(POS[b], POS[a], g)
    # ... and the device model against the ORACLE's mergeNsort_sr_links + runARACNE on that very table (single- and multi-block):
    # same rows in the reference's row order, srp_max to 1e-6 (two different optimisers reach the beta MLE), same ARACNE flags
    tab = dict(pos1=POS[b], pos2=POS[a], clust1=paint[b], clust2=paint[a], len=ln, MI=mi)
    by_clust = [{k: v[(tab["clust1"] == ci) | (tab["clust2"] == ci)] for k, v in tab.items()} for ci in (1, 2, 3)]
    ored, ochk = orc.merge_n_sort_sr_links(by_clust, 3, 20000, 2.0)
    assert len(ored["MI"]) == len(rd)
    for k in ("clust_c", "pos1", "pos2", "clust1", "clust2", "len", "MI"):
        assert np.array_equal(np.asarray(ored[k], dtype=float), rd[k].to_numpy(dtype=float)), k
    assert np.abs(ored["srp_max"] - rd["srp_max"].to_numpy()).max() < 1e-6 * max(1.0, float(np.abs(ored["srp_max"]).max()))
    oflags = orc.run_aracne(ored["pos1"], ored["pos2"], ored["MI"], ochk["pos1"], ochk["pos2"], ochk["MI"])
    assert np.array_equal(oflags.astype(float), rd["ARACNE"].to_numpy())
    qlo, qhi, cnt = engine.sr_len_quantiles(3, 20000, 0.95)
    assert qlo.shape == (3, 19999)
    for ci in (1, 2, 3):
        sel = ((paint[b] == ci) | (paint[a] == ci)) & (ln > 0) & (ln < 20000)
        li = ln[sel].astype(int)
        assert np.array_equal(cnt[ci - 1], np.bincount(li, minlength=20000)[1:20000])
        for l in np.unique(li)[:50]:
            x = np.sort(mi[sel][li == l])
            idx = 1 + (len(x) - 1) * 0.95
            assert qlo[ci - 1, l - 1] == x[int(np.floor(idx)) - 1] and qhi[ci - 1, l - 1] == x[int(np.ceil(idx)) - 1]
        assert np.isnan(qlo[ci - 1][cnt[ci - 1] == 0]).all()
    md = np.full((3, 19999), np.nan)
    md[:, :400] = 0.05 * np.arange(1, 401, dtype=float) ** -0.4     # an arbitrary decay: positional lookup, NaN beyond
    stats = engine.sr_excess_stats(md)
    for ci in (1, 2, 3):
        sel = ((paint[b] == ci) | (paint[a] == ci)) & (ln > 0) & (ln < 20000)
        li = ln[sel].astype(int)
        d = mi[sel] - np.where(li <= 19999, md[ci - 1][np.minimum(li, 19999) - 1], np.nan)
        x = d[d > 0]
        want = [len(x), x.sum(), (x * x).sum(), np.log(x).sum(), np.log1p(-x).sum()]
        np.testing.assert_allclose(stats[ci - 1], want, rtol=1e-12)
    assert np.array_equal(stats, engine.sr_excess_stats(md))     # fixed reduction order: bit-identical on a re-run
    import os
    os.environ["LDW_SR_STATS_PEEL"] = "1"                        # the kernel for any cluster count (per-wave peeling): the same sums in another order
    try:
        peel = engine.sr_excess_stats(md)
        assert np.array_equal(peel, engine.sr_excess_stats(md))
    finally:
        os.environ.pop("LDW_SR_STATS_PEEL")
    np.testing.assert_allclose(peel, stats, rtol=1e-12)
    # p-values: rows below their cluster's crossing of the cut-off are dropped without the continued fraction (r04) — the same reduced set as
    # with every positive excess evaluated (LDW_SR_PVAL_ALL=1), for cut-offs on both sides of the tail's range
    shape = np.array([[0.35, 40.0, 0.0], [0.4, 60.0, 0.0], [0.3, 25.0, 0.0]])
    for k in range(3):
        shape[k, 2] = srp_host._betaln(shape[k, 0], shape[k, 1])
    for cut in (3.0, 0.5, 40.0, -1.0):
        got = engine.sr_pvalues(md, shape, cut)
        red = engine.sr_reduced()
        os.environ["LDW_SR_PVAL_ALL"] = "1"
        try:
            want = engine.sr_pvalues(md, shape, cut)
            red0 = engine.sr_reduced()
        finally:
            os.environ.pop("LDW_SR_PVAL_ALL")
        assert got[:2] == want[:2] and (got[2] == want[2] or (np.isnan(got[2]) and np.isnan(want[2]))), (cut, got, want)
        o, o0 = np.argsort(red["row"]), np.argsort(red0["row"])
        for kk in red:
            assert np.array_equal(np.asarray(red[kk])[o], np.asarray(red0[kk])[o0]), (cut, kk)
        if cut == 3.0:
            assert 0 < got[0] < len(mi)


def _np_len_quantiles(a, b, mi, POS, paint, g, sr_dist, nclust, prob):
    """numpy twin of R/computePairwiseMI.R:417-424 (quantile type 7's two order statistics per cluster and integer len)."""
    S = int(np.ceil(sr_dist)) - 1
    ln = orc.circ_len(POS[b].astype(float), POS[a].astype(float), float(g))
    ok = (ln > 0) & (ln < sr_dist)
    qlo, qhi, cnt = np.full((nclust, S), np.nan), np.full((nclust, S), np.nan), np.zeros((nclust, S), np.int64)
    for ci in range(1, nclust + 1):
        sel = ok & ((paint[b] == ci) | (paint[a] == ci))
        li, x = ln[sel].astype(np.int64), mi[sel]
        o = np.lexsort((x, li))
        li, x = li[o], x[o]
        n = np.bincount(li, minlength=S + 1)[1:S + 1]
        cnt[ci - 1] = n
        start = np.concatenate(([0], np.cumsum(np.bincount(li, minlength=S + 1))))[1:S + 1]
        has = n > 0
        idx = 1 + (n[has] - 1).astype(float) * prob
        qlo[ci - 1, has] = x[start[has] + np.floor(idx).astype(np.int64) - 1]
        qhi[ci - 1, has] = x[start[has] + np.ceil(idx).astype(np.int64) - 1]
    return qlo, qhi, cnt


@pytest.mark.parametrize("nclust", [3, 4, 6])
def test_sr_len_quantiles_select_equals_sort_equals_numpy(engine, synth, nclust):
    """the per-(cluster, len) order statistics by ONE sort (by len) + a radix select per len (k_sr_select, nclust <= 4)
    against the two-sort path (LDW_SR_QUANT_SORT=1; also what nclust = 6 takes) and numpy, over EVERY len, on the engine's own table and on
    tables built to hit the select's corners: all MI of a len equal, ties across the bucket border, a zero and a denormal among ordinary
    values (keys that differ in their top bits), one-row segments, prob 0 / 0.5 / 1 (the two order statistics coincide)."""
    import os
    d = dict(synth)
    rng = np.random.default_rng(7)
    d["paint"] = rng.integers(1, nclust + 1, len(d["POS"])).astype(np.int32)
    _setup(engine, d)
    blocks = orc.make_blocks(512, 1000)
    engine.mi_all_pairs(blocks, sr_dist=3000.0, lr_retain_links=1e6, lr_links_approx=1e5)
    a, b, mi = engine.links(0)
    POS, paint, g = d["POS"], d["paint"], d["g"]

    def check(a, b, mi, probs):
        for prob in probs:
            want = _np_len_quantiles(a, b, mi, POS, paint, g, 3000.0, nclust, prob)
            os.environ.pop("LDW_SR_QUANT_SORT", None)
            got = engine.sr_len_quantiles(nclust, 3000.0, prob)
            os.environ["LDW_SR_QUANT_SORT"] = "1"
            try:
                srt = engine.sr_len_quantiles(nclust, 3000.0, prob)
            finally:
                os.environ.pop("LDW_SR_QUANT_SORT", None)
            for w, x, y, nm in zip(want, got, srt, ("q_lo", "q_hi", "n")):
                assert np.array_equal(w, x, equal_nan=True), (nm, prob, "select")
                assert np.array_equal(w, y, equal_nan=True), (nm, prob, "sort")

    check(a, b, mi, (0.95, 0.5, 0.0, 1.0, 0.999))
    # corners, on the same pairs: (i) few distinct values (long runs of equal keys: buckets of equal keys larger than the LDS candidate
    # array when the table is large enough, ties at the ranks), (ii) values spanning the whole exponent range incl. 0 and a denormal
    mi2 = rng.choice(np.array([0.125, 0.25, 0.25 + 2.0 ** -50, 0.5]), len(mi))
    engine.links_import(0, a, b, mi2)
    check(a, b, mi2, (0.95, 0.5))
    mi3 = np.abs(rng.standard_normal(len(mi))) * 10.0 ** rng.integers(-12, 1, len(mi))
    mi3[rng.integers(0, len(mi), 50)] = 0.0
    mi3[rng.integers(0, len(mi), 50)] = 5e-324
    mi3[rng.integers(0, len(mi), 50)] = -1e-17       # (a rounding-negative MI: the key order must still be the value order)
    engine.links_import(0, a, b, mi3)
    check(a, b, mi3, (0.95, 0.02))
    # (iv) a few lens with 60 000 rows each (rows may repeat a pair: the table is what is imported): buckets beyond the LDS candidate array ->
    # further histogram sweeps; with 4 distinct values the bucket is a run of EQUAL keys larger than the array
    pick = rng.choice(len(mi), 6, replace=False)
    ab, bb = np.repeat(a[pick], 60000), np.repeat(b[pick], 60000)
    big = np.abs(rng.standard_normal(len(ab))) * 0.05
    engine.links_import(0, ab, bb, big)
    check(ab, bb, big, (0.95, 0.5, 1.0))
    big2 = rng.choice(np.array([0.125, 0.25, 0.25 + 2.0 ** -50, 0.5]), len(ab), p=(0.05, 0.6, 0.3, 0.05))
    engine.links_import(0, ab, bb, big2)
    check(ab, bb, big2, (0.95, 0.65, 0.05))
    # (iii) a handful of rows: one-row and two-row segments
    keep = rng.choice(len(mi), 40, replace=False)
    keep.sort()
    engine.links_import(0, a[keep], b[keep], mi[keep])
    check(a[keep], b[keep], mi[keep], (0.95, 0.5))


def test_device_beta_tail_against_scipy(engine, synth):
    """-log P_beta(X > x): the device continued fraction against scipy (mpmath where the tail underflows a double) over
    both branches and deep tails, through ldw_sr_pvalues on a table whose MI values are the probes themselves."""
    from scipy import special
    d = synth
    _setup(engine, d)
    blocks = orc.make_blocks(512, 1000)
    engine.mi_all_pairs(blocks, sr_dist=3000.0, lr_retain_links=1e6, lr_links_approx=1e5)
    a, b, mi = engine.links(0)
    ln = orc.circ_len(d["POS"][b].astype(float), d["POS"][a].astype(float), float(d["g"]))
    qlo, qhi, cnt = engine.sr_len_quantiles(3, 3000.0, 0.95)
    for (sa_, sb_) in ((0.7, 3.0), (1.4, 60.0), (2.5, 900.0), (25.0, 4000.0)):
        md = np.zeros((3, 2999))                              # zero decay: diff = MI itself
        shape = np.tile([sa_, sb_, special.betaln(sa_, sb_)], (3, 1))
        n_red, n_pool, mn = engine.sr_pvalues(md, shape, -1.0)
        red = engine.sr_reduced()
        ok = (ln > 0) & (ln < 3000) & (mi > 0)
        assert n_red == int(ok.sum()) == n_pool and mn == mi[ok].min()
        assert np.array_equal(red["MI"], mi[red["row"]])
        pick = np.argsort(red["MI"])[np.linspace(0, n_red - 1, 400).astype(int)]
        want = orc.neg_log_beta_sf(red["MI"][pick], sa_, sb_)
        np.testing.assert_allclose(red["srp_max"][pick], want, rtol=2e-10, atol=1e-13)
        np.testing.assert_allclose(red["srp_max"], srp_host.neg_log_beta_sf(red["MI"], sa_, sb_), rtol=2e-10, atol=1e-13)
        assert want.max() > 5 * max(want.min(), 1e-3)


def test_sr_only_mode(engine, synth):
    """perform_SR_analysis_only drops SNPs without a short-range partner before each block (non-contiguous,
    non-square blocks -> Q1 scramble differs from the full run)."""
    d = synth
    _setup(engine, d)
    POS, g, sr_dist = d["POS"], d["g"], 3000.0
    blocks = orc.make_blocks(512, 1000)
    engine.links_begin(len(blocks))
    ref = orc.perform_mi_computation(d["states"], POS, g, d["r"], d["uqe"], d["hdw"], d["paint"], 3, sr_dist=sr_dist,
                                     max_blk_sz=1000, sr_only=True, do_srp=False)
    POSf = POS.astype(float)
    for fs, fe, ts, te in blocks:
        fi, ti = np.arange(fs - 1, fe), np.arange(ts - 1, te)
        ln = np.abs(orc.circ_len(POSf[ti][None, :], POSf[fi][:, None], g))
        fi, ti = fi[(ln < sr_dist).any(axis=1)], ti[(ln < sr_dist).any(axis=0)]
        engine.mi_block_links(fi, ti, sr_dist=sr_dist, sr_only=True)
    engine.links_end()
    a, b, mi = engine.links(0)
    assert engine.links_count(1) == 0
    tot = sum(len(x["MI"]) for x in ref.sr_links_by_clust)
    c1, c2 = d["paint"][b], d["paint"][a]
    got = sum(int(((c1 == ci) | (c2 == ci)).sum()) for ci in (1, 2, 3))
    assert got == tot > 0
    sel = (c1 == 1) | (c2 == 1)
    assert np.abs(mi[sel] - ref.sr_links_by_clust[0]["MI"]).max() < MI_TIGHT


def test_elementwise_twins(engine, kat):
    ops = [kat[f"op_{k}"] for k in ("den", "uq", "pxy", "pxpy", "RXY", "pXrX", "pYrY")]
    MI = kat["MI0"].copy()
    engine.fast_hadamard(MI, *ops)
    np.testing.assert_allclose(MI, kat["MI1"], rtol=1e-15, atol=1e-15)   # device log() may differ from libm in the last ulp
    nv = np.ones((5, len(kat["ref_chars"])), order="F")
    engine.acgtn2num(nv, list(kat["ref_chars"]))
    assert np.array_equal(nv, kat["nv"])
    nv0 = np.ones((5, 0), order="F")
    engine.acgtn2num(nv0, [])                  # empty input is a no-op


def test_c2_full_size_properties(engine):
    """BASELINE config 2 (5k SNPs x 1k seqs) at full size: size-independent properties + sampled oracle parity."""
    syn = synth_alignment(5000, 1000, seed=1988)
    st = syn["states"]
    uqe, r = orc.uqe_r(st)
    engine.set_alignment(st)
    hdw = engine.hamming_weights(500)
    assert np.array_equal(hdw, c_oracle.hamming_weights(st, 500))
    d = dict(states=st, hdw=hdw, r=r, uqe=uqe, POS=syn["POS"], paint=syn["paint"], g=float(syn["g"]))
    _setup(engine, d)
    idx = np.arange(5000)
    MI = engine.mi_block(idx, idx, quirk=L.QUIRK_INTENDED)
    assert np.abs(MI - MI.T).max() < 1e-12                      # symmetry
    assert MI.min() > -1e-9                                     # a KL divergence of smoothed tables
    # self-information on the diagonal: MI(a,a) equals the smoothed entropy-like value of the oracle
    rng = np.random.default_rng(4)
    for a, b in zip(rng.integers(0, 5000, 25), rng.integers(0, 5000, 25)):
        assert abs(MI[a, b] - orc.mi_pair_direct(st, hdw, r, uqe, int(a), int(b))) < MI_TIGHT
    # ---- the WHOLE 5000 x 5000 block against the C oracle (block-faithful restatement, reference quirk mode) ----
    Mq = engine.mi_block(idx, idx)
    ref = c_oracle.mi_block(st, hdw, r, uqe, idx, idx)
    assert ref.shape == Mq.shape == (5000, 5000)
    assert np.abs(Mq - ref).max() < MI_TIGHT
    # ---- the COMPLETE link tables against the oracle's a-7 selection on the oracle's MI: same rows, same order ----
    POS, paint, g = syn["POS"], syn["paint"], float(syn["g"])
    approx = MIH.lr_links_approx(POS, g, 20000.0)
    assert approx == orc.lr_links_approx(POS, g, 20000.0)
    bl = orc.block_links(ref, idx, idx, POS, paint, g, 20000.0, 1e6, approx)
    for cold in (True, False):       # a cold pass (probe / plain first block) and a warm one (bucket guess from the pass before)
        if cold:
            engine.reset_speculation()
        engine.mi_all_pairs(MIH.make_blocks(5000, 10000), 20000.0, 1e6, approx)
        stt = engine.block_stats()
        assert stt["n_sr"][0] + stt["n_lr_total"][0] == 5000 * 4999 // 2
        assert stt["n_lr_total"][0] == bl.n_lr_total and stt["n_sr"][0] == len(bl.sr["MI"])
        assert abs(stt["disc_thresh"][0] - bl.disc_thresh) < MI_TIGHT
        sa, sb, smi = engine.links(0)
        assert np.array_equal(sa, bl.sr["a"]) and np.array_equal(sb, bl.sr["b"])       # short-range table: row-exact
        assert np.abs(smi - bl.sr["MI"]).max() < MI_TIGHT
        a, b, mi = engine.links(1)
        assert (a > b).all() and np.all(mi >= stt["disc_thresh"][0])
        key = a.astype(np.int64) + b.astype(np.int64) * 5000
        assert (np.diff(key) > 0).all()                              # reference row order (column-major, a > b)
        # long-range table: the oracle's retained rows, in its order; a pair may sit on either side of `>=` only if its MI is
        # within the parity tolerance of the threshold itself (the epilogue is not bit-matched to the reference's summation order)
        okey = bl.lr["a"].astype(np.int64) + bl.lr["b"].astype(np.int64) * 5000
        both = np.intersect1d(key, okey, assume_unique=True)
        only_dev, only_orc = np.setdiff1d(key, okey, assume_unique=True), np.setdiff1d(okey, key, assume_unique=True)
        # (a tie group — pairs with equivalent joint tables — that holds the order statistic stays together on the device, where
        # equal tables give equal bits, and is split in the last bit by the oracle's A,C,G,T,N summation order: seen here with 49
        # partners of one SNP)
        assert len(only_dev) + len(only_orc) <= max(3, len(okey) // 1000), (len(only_dev), len(only_orc))
        for k in only_dev:
            assert abs(float(mi[key == k][0]) - bl.disc_thresh) < MI_TIGHT
        for k in only_orc:
            assert abs(float(bl.lr["MI"][okey == k][0]) - bl.disc_thresh) < MI_TIGHT
        sel_d, sel_o = np.isin(key, both, assume_unique=True), np.isin(okey, both, assume_unique=True)
        assert np.array_equal(key[sel_d], okey[sel_o])                # same rows in the same order
        assert np.abs(mi[sel_d] - bl.lr["MI"][sel_o]).max() < MI_TIGHT
        assert len(both) > 0.9 * 1e6 * bl.n_lr_total / approx
    # ... and the selection rule itself on the DEVICE's dense MI: quantile type 7 + `>=` give exactly the rows the default path kept
    rr, cc = orc.block_pair_index(5000, 5000, True)
    ln = orc.circ_len(np.asarray(POS, dtype=np.float64)[cc], np.asarray(POS, dtype=np.float64)[rr], g)
    lrm = ln > 20000.0
    vals = Mq[rr[lrm], cc[lrm]]
    thr = orc.quantile7(vals, bl.prob)
    keep = vals >= thr
    assert thr == stt["disc_thresh"][0]
    assert np.array_equal(rr[lrm][keep], a) and np.array_equal(cc[lrm][keep], b) and np.array_equal(vals[keep], mi)


def _dense_block_selection(Md, fi, ti, POS, g, sr_dist, lr_retain, approx, diag):
    """R/computePairwiseMI.R:306-358 on a dense device MI block: (a, b, MI) of the rows `MI >= quantile(MI_lr, prob)` keeps, in the
    reference's row order, the threshold and the number of long-range pairs.  quantile7 is the oracle's (oracle/ldw_oracle.py)."""
    nf, nt = len(fi), len(ti)
    rr, cc = orc.block_pair_index(nf, nt, diag)
    P = np.asarray(POS, dtype=np.float64)
    lrm = orc.circ_len(P[ti][cc], P[fi][rr], g) > sr_dist
    rr, cc = rr[lrm], cc[lrm]
    n_lr = len(rr)
    prob = max(0.0, 1 - ((lr_retain * (n_lr / approx)) / n_lr))
    vals = Md[rr, cc]
    thr = orc.quantile7(vals, prob)
    keep = vals >= thr
    return fi[rr[keep]], ti[cc[keep]], vals[keep], thr, n_lr


def test_c4_blocks_selection_pinned_to_oracle(engine):
    """BASELINE config 4 at full size, one DIAGONAL and one OFF-DIAGONAL 10k x 10k block pair: (i) the dense device MI of the block
    (ldw_mi_block: 5-limb GEMM + fp64 epilogue for every pair) equals the C oracle on a 512 x 512 sub-block (< 1e-10), with the
    block's own Q1 geometry; (ii) the oracle's selection rule (quantile type 7 + `>=`, reference row order) applied to that dense
    MI gives a threshold and a retained (a, b, MI) set that the DEFAULT path (approximate GEMM + screen + popcount sums,
    speculative selection) reproduces exactly — rows, order, MI bits, threshold — cold and warm."""
    import torch
    Ls, N = 100_000, 5_000
    syn = synth_alignment(Ls, N, seed=1988, device="cuda", as_numpy=False)
    st_dev = syn["states"]
    engine.set_alignment(st_dev)
    cnt = engine.state_counts()
    uqe = (cnt > 0).T.astype(np.float64)
    r = uqe.sum(axis=1)
    hdw = engine.hamming_weights(int(Ls * 0.1))
    engine.set_weights(hdw)
    POS, g, paint = syn["POS"], float(syn["g"]), syn["paint"]
    engine.set_snp_meta(r, uqe, POS, paint, g)
    approx = MIH.lr_links_approx(POS, g, 20000.0)
    blocks = MIH.make_blocks(Ls, 10000)
    pick = [0, 30]          # (1..10000) x (1..10000) and an off-diagonal pair in the middle of the list: (30001..40000) x (60001..70000)
    assert blocks[pick[0]].tolist() == [1, 10000, 1, 10000] and blocks[pick[1]][0] != blocks[pick[1]][2]
    sub = blocks[pick]
    want = []
    for fs, fe, ts, te in sub.tolist():
        fi, ti = np.arange(fs - 1, fe), np.arange(ts - 1, te)
        diag = fs == ts
        Md = engine.mi_block(fi, ti)                       # dense, reference quirk mode (square block: RXY = r[b] r[a] / 4)
        # (i) 512 x 512 sub-block against the C oracle: the oracle's Q1 index depends on the block shape, so the sub-block is
        # checked in INTENDED mode (RXY = r_a r_b / 4, shape-free) and the quirk is checked per pair below
        Mi = engine.mi_block(fi, ti, quirk=L.QUIRK_INTENDED)
        o_f, o_t = 3000, (3000 if diag else 6100)
        sf, stt_ = fi[o_f:o_f + 512], ti[o_t:o_t + 512]
        rows_needed = np.unique(np.concatenate([sf, stt_]))
        st_sub = st_dev[torch.as_tensor(rows_needed, device=st_dev.device)].cpu().numpy()
        loc_f, loc_t = np.searchsorted(rows_needed, sf), np.searchsorted(rows_needed, stt_)
        # intended mode == the oracle's block-faithful MI of a SYMMETRIC geometry: evaluate the oracle on (sf u st) x (sf u st) and cut
        allr = np.arange(len(rows_needed))
        Mo = c_oracle.mi_block(st_sub, hdw, r[rows_needed], uqe[rows_needed], allr, allr)    # square: Q1 harmless up to transposition
        # square block with from == to: RXY[c] = r[c / n] r[c % n] / 4 = r_a r_b / 4 (symmetric in a, b)
        assert np.abs(Mi[o_f:o_f + 512, o_t:o_t + 512] - Mo[np.ix_(loc_f, loc_t)]).max() < MI_TIGHT
        rng = np.random.default_rng(31)
        for _ in range(16):   # the reference's Q1 RXY of THIS block geometry, per pair
            a_l, b_l = int(rng.integers(0, len(fi))), int(rng.integers(0, len(ti)))
            rows2 = st_dev[[int(fi[a_l]), int(ti[b_l])]].cpu().numpy()
            rxy = orc.q1_rxy(a_l, b_l, len(fi), len(ti), r[fi], r[ti])
            refv = orc.mi_pair_direct(rows2, hdw, r[[fi[a_l], ti[b_l]]], uqe[[fi[a_l], ti[b_l]]], 0, 1, rxy)
            assert abs(Md[a_l, b_l] - refv) < MI_TIGHT
        # (ii) the oracle's selection on the dense device MI
        want.append(_dense_block_selection(Md, fi, ti, POS, g, 20000.0, 1e6, approx, diag))
        del Md, Mi
    for cold in (True, False):
        if cold:
            engine.reset_speculation()
        c0 = engine.counters()
        engine.mi_all_pairs(sub, 20000.0, 1e6, approx)
        c1 = engine.counters()
        assert c1["apx_blocks"] - c0["apx_blocks"] >= (1 if cold else 2)       # the default path, not a fallback
        stt = engine.block_stats()
        la, lb, lmi = engine.links(1)
        off = 0
        for bi, (wa, wb, wmi, thr, n_lr) in enumerate(want):
            n = int(stt["n_lr_kept"][bi])
            assert int(stt["n_lr_total"][bi]) == n_lr
            assert stt["disc_thresh"][bi] == thr, (bi, cold, stt["disc_thresh"][bi], thr)
            assert n == len(wmi), (bi, cold, n, len(wmi))
            assert np.array_equal(la[off:off + n], wa) and np.array_equal(lb[off:off + n], wb), (bi, cold)
            assert np.array_equal(lmi[off:off + n], wmi), (bi, cold)
            off += n
        assert off == len(lmi)


def test_speculative_gather_and_fallback(engine, synth):
    """From the second block on, the epilogue gathers long-range candidates itself using the previous block's
    histogram bucket as a guess; a guess that turns out too high must fall back to the dense gather.  Three blocks:
    same filter twice (guess holds), then keep-everything (true bucket 0 < guess -> fallback)."""
    _setup(engine, synth)
    POS, g = synth["POS"], synth["g"]
    approx = orc.lr_links_approx(POS, g, 20000.0)
    plan = [(np.arange(0, 200), np.arange(200, 400), 300.0), (np.arange(100, 300), np.arange(300, 500), 300.0),
            (np.arange(0, 256), np.arange(256, 512), 1e12), (np.arange(0, 300), np.arange(0, 300), 250.0)]
    engine.links_begin(len(plan))
    for fi, ti, retain in plan:
        engine.mi_block_links(fi, ti, lr_retain_links=retain, lr_links_approx=approx)
    engine.links_end()
    st = engine.block_stats()
    a, b, mi = engine.links(1)
    off = 0
    for bi, (fi, ti, retain) in enumerate(plan):
        Mb = c_oracle.mi_block(synth["states"], synth["hdw"], synth["r"], synth["uqe"], fi, ti)
        bl = orc.block_links(Mb, fi, ti, POS, synth["paint"], g, 20000.0, retain, approx)
        n = len(bl.lr["MI"])
        assert st["n_lr_total"][bi] == bl.n_lr_total and st["n_lr_kept"][bi] == n, (bi, st["n_lr_kept"][bi], n)
        assert np.array_equal(a[off:off + n], bl.lr["a"]) and np.array_equal(b[off:off + n], bl.lr["b"]), bi
        assert np.abs(mi[off:off + n] - bl.lr["MI"]).max() < MI_TIGHT
        off += n
    assert off == len(mi)
    assert st["n_lr_kept"][2] == st["n_lr_total"][2] > 10 * st["n_lr_kept"][1]   # block 3 kept everything


def _lr_blocks(links, stats):
    """Split a long-range table into per-block dicts {(a, b): MI}."""
    a, b, mi = links
    out, off = [], 0
    for n in stats["n_lr_kept"].tolist():
        out.append(dict(zip(zip(a[off:off + n].tolist(), b[off:off + n].tolist()), mi[off:off + n].tolist())))
        off += n
    assert off == len(mi)
    return out


def _same_up_to_threshold_ties(d0, d1, thr, tol):
    """Two retained sets of one block agree except for pairs whose MI sits on the quantile threshold itself: pairs
    with equivalent joint tables tie there, and which side of `>=` a tie lands on depends on the last bit of an fp64
    sum whose order is not the reference's either (the epilogue is not bit-matched)."""
    for k in set(d0) ^ set(d1):
        v = d0.get(k, d1.get(k))
        assert abs(v - thr) < tol, (k, v, thr)
    for k in set(d0) & set(d1):
        assert abs(d0[k] - d1[k]) < tol, (k, d0[k], d1[k])


@pytest.mark.parametrize("fused", [False])   # (ldw_set_fused(0), what bench.py calls, is still accepted; 1 was removed)
def test_fp32_screen_loses_nothing(engine, synth, fused):
    """The fp32 screen in front of the fp64 MI evaluation (speculative blocks) must never dismiss a pair that the exact
    value would have emitted: mode 2 evaluates every pair both ways and counts such pairs; and since every emitted MI
    is the exact one, the link tables with the screen on are bit-identical to those with the screen off."""
    syn = synth_alignment(3000, 700, seed=11)
    st = syn["states"]
    uqe, r = orc.uqe_r(st)
    engine.set_alignment(st)
    hdw = engine.hamming_weights(300)
    d = dict(states=st, hdw=hdw, r=r, uqe=uqe, POS=syn["POS"], paint=syn["paint"], g=float(syn["g"]))
    _setup(engine, d)
    approx = MIH.lr_links_approx(syn["POS"], float(syn["g"]), 20000.0)
    blocks = MIH.make_blocks(3000, 1000)     # 6 block pairs, 3 of them diagonal
    engine.set_fused(fused)
    out = {}
    for mode in (0, 1, 2):
        engine.set_screen(mode)
        c0 = engine.counters()
        for _ in range(2):
            engine.mi_all_pairs(blocks, 20000.0, 20000.0, approx)
        c1 = engine.counters()
        out[mode] = (engine.links(0), engine.links(1), c1["screen_violations"] - c0["screen_violations"],
                     c1["spec_misses"] - c0["spec_misses"])
    engine.set_screen(1)
    assert out[2][2] == 0, f"the screen would have lost {out[2][2]} pairs"
    assert out[1][3] == 0 and out[0][3] == 0     # the second pass runs speculatively, i.e. with the screen
    for which in (0, 1):
        for mode in (1, 2):
            for x, y in zip(out[0][which], out[mode][which]):
                assert np.array_equal(x, y), (which, mode)
    assert len(out[0][1][2]) > 15000 and len(out[0][0][2]) > 0


def _tables_as_dicts(engine, POS):
    out = []
    for which in (1, 0):
        a, b, mi = engine.links(which)
        out.append(dict(pos1=POS[b].astype(np.int64), pos2=POS[a].astype(np.int64), MI=mi, a=a, b=b))
    return out   # lr, sr


@pytest.mark.parametrize("min_links", [5000, 300])
def test_lr_tukey_and_aracne_match_oracle(engine, synth, min_links):
    """analyse_long_range_links' numeric core on the device-resident tables (quantiles type 7,
    Tukey thresholds, the top-links fallback, outlier set, ARACNE against rbind(lr, sr)[MI > thr]) vs the oracle.  The sr
    part of the pool is what sr_links.tsv holds — the REDUCED short-range set (R/lr_analyser.R:67, R/computePairwiseMI.R:140),
    here a strict subset of the engine's raw short-range table so that pooling the raw table would be noticed."""
    _setup(engine, synth)
    POS, g = synth["POS"], synth["g"]
    approx = orc.lr_links_approx(POS, g, 20000.0)
    engine.mi_all_pairs(np.array(orc.make_blocks(512, 200), dtype=np.int32), 20000.0, 6000.0, approx)
    lr, sr_all = _tables_as_dicts(engine, POS)
    assert len(lr["MI"]) >= 5000
    keep = (np.arange(len(sr_all["MI"])) * 2654435761 % 7) < 3           # stands for srp_max > srp_cutoff
    sr = {k: v[keep] for k, v in sr_all.items()}
    ref = orc.analyse_long_range_links({k: lr[k] for k in ("pos1", "pos2", "MI")}, sr, min_links=min_links)
    ref_all = orc.analyse_long_range_links({k: lr[k] for k in ("pos1", "pos2", "MI")}, sr_all, min_links=min_links)
    assert ref_all["n_pool"] > ref["n_pool"]                             # the raw table would pool more rows
    info = engine.lr_tukey(min_links, sr=(sr["a"], sr["b"], sr["MI"]))
    assert info["fallback"] == ref["fallback"] == (min_links == 5000)
    assert np.array_equal(info["q13"], ref["q13"]) and np.array_equal(info["thresholds"], ref["thresholds"])   # same order statistics, same arithmetic
    assert info["n_red"] == len(ref["rows"]) > 0 and info["n_pool"] == ref["n_pool"]
    red = engine.lr_reduced()
    flags = engine.aracne_device()
    o = np.argsort(-red["MI"], kind="stable")
    assert np.array_equal(red["row"][o], ref["rows"])
    assert np.array_equal(flags[o], ref["ARACNE"])
    assert 0 < flags.sum() < len(flags)          # both outcomes occur
    # the host mirror with the reference's column layout
    from ldweaver_amd import lr as LR
    sd = SnpDat(states=synth["states"], POS=POS, g=g, uqe=synth["uqe"], r=synth["r"])
    with pytest.warns(UserWarning) if ref["fallback"] else np.errstate():
        out = LR.analyse_long_range_links(engine, sd, pd.DataFrame({k: sr[k] for k in ("pos1", "pos2", "MI")}),
                                          CdsVar(paint=synth["paint"], nclust=3), min_links=min_links)
    df = out["lr_links_red"]
    assert list(df.columns) == ["pos1", "pos2", "clust1", "clust2", "len", "MI", "ARACNE"]
    assert np.array_equal(df["pos1"].to_numpy(), ref["red"]["pos1"]) and np.array_equal(df["ARACNE"].to_numpy().astype(bool), ref["ARACNE"])


def test_ldmap_matches_oracle(engine, synth):
    """genomewide_LDMap's numeric core (rank of positions, block sums with the .mat kernel, log10, rescale) vs the
    oracle; genome-wide with an explicit reducer and windowed with the default one refused / accepted like the reference."""
    _setup(engine, synth)
    POS, g = synth["POS"], synth["g"]
    approx = orc.lr_links_approx(POS, g, 20000.0)
    engine.mi_all_pairs(np.array(orc.make_blocks(512, 200), dtype=np.int32), 20000.0, 6000.0, approx)
    lr, sr = _tables_as_dicts(engine, POS)
    for reducer, win in ((7, None), (16, None), (5, (int(POS[40]), int(POS[400])))):
        ref = orc.ld_map(lr, sr, reducer=reducer, from_=win[0] if win else None, to=win[1] if win else None)
        htm, n_pos, r = engine.ldmap(reducer, *(win or (0, 0)))
        assert n_pos == len(ref["pos_vec"]) and r == ref["reducer"] and htm.shape == ref["htm"].shape
        assert np.abs(htm - ref["htm"]).max() < 1e-12      # fp64 atomics: summation order differs
        assert htm.min() == 0.0 and htm.max() == 1.0 and np.array_equal(htm, htm.T)
    with pytest.raises(RuntimeError):
        engine.ldmap(0)          # default reducer round(512 / 1000) = 1 <= 1: the unreduced branch is refused
    # r05: snp.dat$POS in ANY order and positions held by two SNPs — the rank of a position is its rank among the sorted
    # DISTINCT positions (R/LDSummaryPlot.R:57: sort(unique(c(pos1, pos2)))), not the SNP index.  The same links under a permutation of the SNPs,
    # then with repeated positions, against the oracle on the positions themselves
    rng = np.random.default_rng(5)
    perm = rng.permutation(512)
    inv = np.empty(512, dtype=np.int32)
    inv[perm] = np.arange(512, dtype=np.int32)
    tabs = [engine.links(w) for w in (0, 1)]
    for label, POS2 in (("permuted", POS[perm]), ("repeated", np.repeat(POS[::2], 2)[perm])):
        engine.set_snp_meta(synth["r"][perm], synth["uqe"][perm], POS2, synth["paint"][perm], g)
        for w in (0, 1):
            a, b, mi = tabs[w]
            engine.links_import(w, inv[a], inv[b], mi)
        lr2, sr2 = _tables_as_dicts(engine, POS2)
        for reducer, win in ((7, None), (5, (int(POS[40]), int(POS[400])))):
            ref = orc.ld_map(lr2, sr2, reducer=reducer, from_=win[0] if win else None, to=win[1] if win else None)
            htm, n_pos, r = engine.ldmap(reducer, *(win or (0, 0)))
            assert n_pos == len(ref["pos_vec"]) and r == ref["reducer"] and htm.shape == ref["htm"].shape, label
            assert np.abs(htm - ref["htm"]).max() < 1e-12 and np.array_equal(htm, htm.T), label
        if label == "repeated":
            assert n_pos <= 256


def test_mixed_precision_gemm_is_exact(engine, synth):
    """Mixed-precision path: block-wide GEMM with the 3 high weight limbs, low limbs from the gathered GEMM for the units
    the screen lists.  The joint sums it feeds the fp64 evaluation are the same integers as the 5-limb GEMM's, so the
    link tables must be BIT-identical to the plain path; the widened screen must lose nothing (verify mode)."""
    syn = synth_alignment(3000, 700, seed=5)
    st = syn["states"]
    uqe, r = orc.uqe_r(st)
    engine.set_alignment(st)
    hdw = engine.hamming_weights(300)
    d = dict(states=st, hdw=hdw, r=r, uqe=uqe, POS=syn["POS"], paint=syn["paint"], g=float(syn["g"]))
    _setup(engine, d)
    approx = MIH.lr_links_approx(syn["POS"], float(syn["g"]), 20000.0)
    blocks = MIH.make_blocks(3000, 1000)
    out = {}
    engine.set_path(1)     # the limb paths (auto would take the approximate-GEMM path on these weights)
    for mixed, scr in ((False, 1), (True, 1), (True, 2)):
        engine.set_mixed(mixed)
        engine.set_screen(scr)
        c0 = engine.counters()
        for _ in range(2):
            engine.mi_all_pairs(blocks, 20000.0, 20000.0, approx)
        c1 = engine.counters()
        out[(mixed, scr)] = (engine.links(0), engine.links(1), {k: c1[k] - c0[k] for k in c1})
    engine.set_mixed(True)
    engine.set_screen(1)
    engine.set_path(0)
    assert out[(False, 1)][2]["mixed_blocks"] == 0 and out[(True, 1)][2]["mixed_blocks"] >= len(blocks)
    assert out[(True, 2)][2]["screen_violations"] == 0
    for which in (0, 1):
        for key in ((True, 1), (True, 2)):
            for x, y in zip(out[(False, 1)][which], out[key][which]):
                assert np.array_equal(x, y), (which, key)
    assert len(out[(True, 1)][1][2]) > 15000


def test_perform_mi_computation_two_ranks(engine, sample, tmp_path):
    """SURVEY 8e end to end: perform_MI_computation under torch.distributed with 2 ranks (gloo, both engines on this box's
    one GPU): blocks dealt over the ranks, one gather, rank 0 adopts the assembled tables (ldw_links_import) and runs the
    short-range model + ARACNE on them.  Files and frame must equal the single-process run's."""
    import subprocess
    import pandas as pd
    sd = SnpDat.from_states(sample["states"], sample["POS"], sample["g"])
    one = tmp_path / "one"
    two = tmp_path / "two"
    one.mkdir()
    two.mkdir()
    red1 = MIH.perform_MI_computation(sd, sample["hdw"], CdsVar(paint=sample["paint"], nclust=3), ncores=1,
                                      lr_save_path=str(one / "lr_links.tsv"), sr_save_path=str(one / "sr_links.tsv"),
                                      plt_folder=str(one / "PLOTS"), max_blk_sz=1000, lr_retain_links=1e5, engine=engine, verbose=False,
                                      quirk_mode=L.QUIRK_INTENDED)   # ragged blocks: Q1 scrambles RXY there, the srp fit has no solution
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29533", os.path.join(os.path.dirname(__file__), "dist_worker.py"), str(two)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (one / "lr_links.tsv").read_bytes() == (two / "lr_links.tsv").read_bytes()
    _frames_equal(red1, pd.read_pickle(two / "red.pkl"))


@pytest.mark.parametrize("nproc", [2, 3])
def test_perform_mi_computation_ranks_keep_their_short_range_rows(engine, sample, tmp_path, nproc):
    """VERDICT r04 item 6 end to end: perform_MI_computation(sr_tail="dist") under 2 and 3 gloo ranks — only the long-range table is gathered,
    the short-range model + ARACNE run over the ranks (dist_srp) — against the single-process run: BOTH files byte-identical (the excess
    statistics are summed per reference block in make_blocks order on every route), the frame equal."""
    import pandas as pd
    sd = SnpDat.from_states(sample["states"], sample["POS"], sample["g"])
    one, two = tmp_path / "one", tmp_path / "many"
    one.mkdir()
    two.mkdir()
    red1 = MIH.perform_MI_computation(sd, sample["hdw"], CdsVar(paint=sample["paint"], nclust=3), ncores=1,
                                      lr_save_path=str(one / "lr_links.tsv"), sr_save_path=str(one / "sr_links.tsv"),
                                      plt_folder=str(one / "PLOTS"), max_blk_sz=1000, lr_retain_links=1e5, engine=engine, verbose=False,
                                      quirk_mode=L.QUIRK_INTENDED)
    r = _torchrun(nproc, 29543 + nproc, "dist_worker.py", two, "rows_stay")
    assert r.returncode == 0, r.stderr[-3000:]
    assert (one / "lr_links.tsv").read_bytes() == (two / "lr_links.tsv").read_bytes()
    assert (one / "sr_links.tsv").read_bytes() == (two / "sr_links.tsv").read_bytes()
    _frames_equal(red1, pd.read_pickle(two / "red.pkl"))
    for k in (1, 2, 3):
        assert (one / "PLOTS" / f"c{k}_fit_data.tsv").read_bytes() == (two / "PLOTS" / f"c{k}_fit_data.tsv").read_bytes()


def _frames_equal(red1, red2):
    assert list(red1.columns) == list(red2.columns) and len(red1) == len(red2) > 0
    for c in red1.columns:
        a, b = red1[c].to_numpy(), red2[c].to_numpy()
        assert np.array_equal(a, b) if a.dtype.kind in "iub" else np.allclose(a, b, rtol=0, atol=1e-9), c


def _torchrun(nproc, port, script, *args, timeout=300, env=None):
    import subprocess
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **(env or {}))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(os.path.dirname(__file__), script), *map(str, args)]
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)


def test_sr_only_two_ranks(engine, sample, tmp_path):
    """perform_SR_analysis_only under 2 ranks (R/computePairwiseMI.R:179-189 per block, blocks dealt over the ranks, blocks
    left without sites skipped on their owner): frame and sr file equal the single-process run's, no lr file is written."""
    import pandas as pd
    sd = SnpDat.from_states(sample["states"], sample["POS"], sample["g"])
    one, two = tmp_path / "one", tmp_path / "two"
    one.mkdir()
    two.mkdir()
    red1 = MIH.perform_MI_computation(sd, sample["hdw"], CdsVar(paint=sample["paint"], nclust=3), ncores=1,
                                      lr_save_path=str(one / "lr_links.tsv"), sr_save_path=str(one / "sr_links.tsv"),
                                      plt_folder=str(one / "PLOTS"), max_blk_sz=1000, lr_retain_links=1e5, engine=engine, verbose=False,
                                      perform_SR_analysis_only=True, sr_dist=3000, quirk_mode=L.QUIRK_INTENDED)
    r = _torchrun(2, 29535, "dist_worker.py", two, "sr_only")
    assert r.returncode == 0, r.stderr[-2000:]
    assert not (one / "lr_links.tsv").exists() and not (two / "lr_links.tsv").exists()
    assert (one / "sr_links.tsv").read_bytes() == (two / "sr_links.tsv").read_bytes()
    _frames_equal(red1, pd.read_pickle(two / "red.pkl"))
    # r05: ... and with the rows left on their ranks (filtered site lists per block: the model over ranks only needs every block's row count)
    three = tmp_path / "three"
    three.mkdir()
    r = _torchrun(2, 29539, "dist_worker.py", three, "sr_only_rows_stay")
    assert r.returncode == 0, r.stderr[-2000:]
    assert not (three / "lr_links.tsv").exists()
    assert (one / "sr_links.tsv").read_bytes() == (three / "sr_links.tsv").read_bytes()
    _frames_equal(red1, pd.read_pickle(three / "red.pkl"))


def test_failing_rank_is_agreed_on(tmp_path):
    """One rank cannot compute its share: every rank raises (one all-reduce of a status flag before the gather) instead of
    the healthy ranks waiting in a collective for ever."""
    r = _torchrun(2, 29537, "dist_worker.py", tmp_path, "fail", timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    m0, m1 = (tmp_path / "raised_0.txt").read_text(), (tmp_path / "raised_1.txt").read_text()
    assert "failed on rank(s) [1]" in m0 and "failed on rank(s) [1]" in m1, (m0, m1)


def test_rccl_single_rank_walk(engine, sample, tmp_path):
    """The RCCL branch of every dist.py function on GPU tensors (backend "nccl", one rank, collectives forced) and
    perform_MI_computation / estimate_Hamming_distance_weights on top of it: same files and frame as without torch.distributed."""
    import subprocess
    import pandas as pd
    sd = SnpDat.from_states(sample["states"], sample["POS"], sample["g"])
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29541")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "rccl_worker.py"), str(tmp_path)], env=env,
                       capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stderr[-3000:]
    rep = json.load(open(tmp_path / "report.json"))
    assert rep["backend"] == "nccl" and rep["gather_rows"]["sr"] > 0
    for tag, sr_only in (("full", False), ("sr", True)):
        one = tmp_path / f"one_{tag}"
        one.mkdir()
        red1 = MIH.perform_MI_computation(sd, sample["hdw"], CdsVar(paint=sample["paint"], nclust=3), ncores=1,
                                          lr_save_path=str(one / "lr.tsv"), sr_save_path=str(one / "sr.tsv"), plt_folder=str(one / "P"),
                                          max_blk_sz=1000, lr_retain_links=1e5, engine=engine, verbose=False,
                                          perform_SR_analysis_only=sr_only, sr_dist=(3000 if sr_only else 20000), quirk_mode=L.QUIRK_INTENDED)
        _frames_equal(red1, pd.read_pickle(tmp_path / f"red_{tag}.pkl"))
        assert (one / "sr.tsv").read_bytes() == (tmp_path / f"sr_{tag}.tsv").read_bytes()
        if not sr_only:
            assert (one / "lr.tsv").read_bytes() == (tmp_path / "lr_full.tsv").read_bytes()
            # r05: ... and with the short-range rows left on their rank (sr_tail="dist": dist_srp's exchanges on RCCL tensors)
            assert (one / "sr.tsv").read_bytes() == (tmp_path / "sr_rows_stay.tsv").read_bytes()
            assert (one / "lr.tsv").read_bytes() == (tmp_path / "lr_rows_stay.tsv").read_bytes()
            _frames_equal(red1, pd.read_pickle(tmp_path / "red_rows_stay.pkl"))
            assert rep["sr_tail_bytes_sent"]["candidates"] > 0 and rep["sr_tail_bytes_sent"]["kept_links_and_pool"] > 0


def test_screen_and_mixed_paths_on_multiallelic_alignment(engine):
    """Stress for the generic screen (k_mi_screen_generic), the class-4 row slots of the gathered low-limb GEMM and the
    predicated fp64 kernel: an alignment where a third of the SNPs have 3-5 states at sizeable frequencies, some are
    monomorphic, and the weights are irregular.  Screen + mixed precision (default) against the plain path (5-limb GEMM, fp64
    for every pair): link tables bit-identical; verify mode: nothing lost."""
    rng = np.random.default_rng(77)
    Ls, N = 2600, 640
    st = np.zeros((Ls, N), dtype=np.uint8)
    for a in range(Ls):
        k = rng.integers(0, 10)
        if k == 0:
            st[a] = rng.integers(0, 5)                                   # monomorphic
        elif k <= 3:
            st[a] = rng.choice(5, size=N, p=rng.dirichlet(np.ones(5)))   # up to 5 states
        else:
            maj, mnr = rng.choice(5, size=2, replace=False)
            st[a] = np.where(rng.random(N) < rng.uniform(0.05, 0.5), mnr, maj)
        if a % 3 == 1:                                                   # LD with the previous SNP
            keep = rng.random(N) < 0.9
            st[a] = np.where(keep, st[a - 1], st[a])
    uqe, r = orc.uqe_r(st)
    POS = np.sort(rng.choice(np.arange(1, 400000), size=Ls, replace=False)).astype(np.int32)
    hdw = 1.0 / rng.integers(1, 40, size=N).astype(np.float64)
    d = dict(states=st, hdw=hdw, r=r, uqe=uqe, POS=POS, paint=rng.integers(1, 4, Ls).astype(np.int32), g=400000.0)
    _setup(engine, d)
    approx = orc.lr_links_approx(POS, d["g"], 20000.0)
    blocks = np.array(orc.make_blocks(Ls, 1000), dtype=np.int32)       # 1000, 1000, 600: ragged last column -> intended quirk mode
    out = {}
    assert engine.apx_info()["usable"]
    for key, (mixed, scr, path) in dict(plain=(False, 0, 1), fast=(True, 1, 1), verify=(True, 2, 1), apx=(True, 1, 2), apx_verify=(True, 2, 2)).items():
        engine.set_mixed(mixed)
        engine.set_screen(scr)
        engine.set_path(path)
        c0 = engine.counters()
        for _ in range(2):
            engine.mi_all_pairs(blocks, 20000.0, 30000.0, approx, quirk=L.QUIRK_INTENDED)
        c1 = engine.counters()
        out[key] = (engine.links(0), engine.links(1), {k: c1[k] - c0[k] for k in c1})
    engine.set_mixed(True)
    engine.set_screen(1)
    engine.set_path(0)
    assert out["fast"][2]["mixed_blocks"] >= len(blocks) and out["verify"][2]["screen_violations"] == 0
    assert out["apx"][2]["apx_blocks"] >= len(blocks) and out["apx"][2]["mixed_blocks"] == 0 and out["apx_verify"][2]["screen_violations"] == 0
    assert out["apx"][2]["apx_units_listed"] > 0 and out["apx"][2]["apx_pairs_listed"] > 0
    for which in (0, 1):
        for key in ("fast", "verify", "apx", "apx_verify"):
            for x, y in zip(out["plain"][which], out[key][which]):
                assert np.array_equal(x, y), (which, key)
    assert len(out["plain"][1][2]) > 20000 and len(out["plain"][0][2]) > 1000
    # and the plain path itself against the oracle on one off-diagonal block
    fi, ti = np.arange(0, 1000), np.arange(1000, 2000)
    Mg = engine.mi_block(fi, ti, quirk=L.QUIRK_INTENDED)
    Mo = np.array([[orc.mi_pair_direct(st, hdw, r, uqe, int(a), int(b)) for b in (1000, 1500, 1999)] for a in (0, 3, 500, 999)])
    assert np.abs(Mg[np.ix_([0, 3, 500, 999], [0, 500, 999])] - Mo).max() < MI_TIGHT


def test_epilogue_split_equals_the_one_kernel_epilogue(engine):
    """r06: the plain path's fp64 epilogue is two kernels — k_mi_epilogue_fast (straight-line code: tiles and columns of SNPs with 1 or 2 fully
    flagged minor states) and k_mi_epilogue_rest (the units it lists: everything else, predicated code) — against the one-kernel epilogue
    (LDW_NO_EPI_SPLIT): every unit evaluated exactly once and by the same arithmetic, so link tables and dense blocks are equal BIT FOR BIT.
    The alignment mixes all kinds: biallelic SNPs, 3-5 states, monomorphic ones, and uqe that disagrees with the data (a tile of
    one-row SNPs with an unflagged slot is not 'full': the whole tile goes to the list)."""
    rng = np.random.default_rng(606)
    Ls, N = 2300, 520
    st = np.zeros((Ls, N), dtype=np.uint8)
    for a in range(Ls):
        k = rng.integers(0, 12)
        if k == 0:
            st[a] = rng.integers(0, 5)
        elif k <= 2:
            st[a] = rng.choice(5, size=N, p=rng.dirichlet(np.ones(5)))
        elif k <= 4:
            s3 = rng.choice(5, size=3, replace=False)
            st[a] = s3[rng.choice(3, size=N, p=(0.7, 0.2, 0.1))]
        else:
            maj, mnr = rng.choice(5, size=2, replace=False)
            st[a] = np.where(rng.random(N) < rng.uniform(0.05, 0.5), mnr, maj)
    uqe, r = orc.uqe_r(st)
    for a in rng.choice(Ls, size=40, replace=False):          # uqe that disagrees with the data
        present = np.flatnonzero(uqe[a] > 0)
        if rng.random() < 0.5 and len(present) > 1:
            uqe[a, rng.choice(present)] = 0.0                  # present but masked
        else:
            uqe[a, rng.integers(0, 5)] = 1.0                   # (possibly) flagged but absent
    r = uqe.sum(axis=1)
    POS = np.sort(rng.choice(np.arange(1, 300000), size=Ls, replace=False)).astype(np.int32)
    hdw = 1.0 / rng.integers(1, 30, size=N).astype(np.float64)
    d = dict(states=st, hdw=hdw, r=r, uqe=uqe, POS=POS, paint=rng.integers(1, 4, Ls).astype(np.int32), g=300000.0)
    _setup(engine, d)
    approx = orc.lr_links_approx(POS, d["g"], 20000.0)
    blocks = np.array(orc.make_blocks(Ls, 1000), dtype=np.int32)
    fi, ti = np.arange(0, 1000), np.arange(1000, 2300)
    out = {}
    engine.set_mixed(False)
    engine.set_screen(0)
    engine.set_path(1)
    try:
        for key in ("split", "one"):
            if key == "one":
                os.environ["LDW_NO_EPI_SPLIT"] = "1"
            else:
                os.environ.pop("LDW_NO_EPI_SPLIT", None)
            tabs = {}
            for quirk in (L.QUIRK_INTENDED, L.QUIRK_REFERENCE):
                engine.mi_all_pairs(blocks, 20000.0, 30000.0, approx, quirk=quirk)
                tabs[quirk] = (engine.links(0), engine.links(1), engine.block_stats())
            out[key] = (tabs, engine.mi_block(fi, ti), engine.mi_block(fi, fi), engine.mi_block(np.arange(Ls), np.arange(Ls), quirk=L.QUIRK_INTENDED))
    finally:
        os.environ.pop("LDW_NO_EPI_SPLIT", None)
        engine.set_mixed(True)
        engine.set_screen(1)
        engine.set_path(0)
    for quirk in (L.QUIRK_INTENDED, L.QUIRK_REFERENCE):
        a, b = out["split"][0][quirk], out["one"][0][quirk]
        for which in (0, 1):
            for x, y in zip(a[which], b[which]):
                assert np.array_equal(x, y), (quirk, which)
        for k in ("n_lr_total", "n_lr_kept", "n_sr", "disc_thresh"):
            assert np.array_equal(a[2][k], b[2][k]), (quirk, k)
        assert len(a[0][2]) > 1000 and len(a[1][2]) > 10000
    for k in (1, 2, 3):
        assert np.array_equal(out["split"][k], out["one"][k]), k
    # and the split epilogue against the oracle: rows of every kind at columns of every kind
    rows = np.concatenate([np.flatnonzero(r == k)[:3] for k in (1, 2, 3, 4, 5) if (r == k).any()])
    cols = np.concatenate([np.flatnonzero(r == k)[-3:] for k in (1, 2, 3, 4, 5) if (r == k).any()])
    Mo = np.array([[orc.mi_pair_direct(st, hdw, r, uqe, int(a), int(b)) for b in cols] for a in rows])
    assert np.abs(out["split"][3][np.ix_(rows, cols)] - Mo).max() < MI_TIGHT


def test_616_distinct_weights_take_the_approximate_path(engine):
    """The weight structure of BASELINE config 3 at its worst: N = 616 sequences with 616 DISTINCT Hamming weights 1 / (k + 1)
    (R/performPopulationStuctureCorrection.R:76: hdw = 1 / (#neighbours + 1); a real alignment has up to N distinct values, not
    the few clonal classes of the synthetic one).  The approximate-GEMM path must engage (ldw_path_report says which path the
    blocks took and which gate failed otherwise), the verify mode must count no lost pair, and the tables must equal the plain path's."""
    syn = synth_alignment(24000, 616, seed=616)
    st = syn["states"]
    uqe, r = orc.uqe_r(st)
    hdw = 1.0 / (np.random.default_rng(616).permutation(616) + 1.0)
    assert len(np.unique(hdw)) == 616
    d = dict(states=st, hdw=hdw, r=r, uqe=uqe, POS=syn["POS"], paint=syn["paint"], g=float(syn["g"]))
    _setup(engine, d)
    info = engine.apx_info()
    rep0 = engine.path_report()
    assert info["usable"] and rep0["apx_gate"] == "ok (block exponents per 32 positions)" and info["classes"] >= 600, (info, rep0)
    approx = MIH.lr_links_approx(syn["POS"], float(syn["g"]), 20000.0)
    blocks = MIH.make_blocks(24000, 8000)           # 6 block pairs, 3 diagonal
    out = {}
    for key, (mixed, scr, path) in dict(plain=(False, 0, 1), verify=(True, 2, 2), fast=(True, 1, 0)).items():
        engine.set_mixed(mixed)
        engine.set_screen(scr)
        engine.set_path(path)
        engine.reset_speculation()
        c0, p0 = engine.counters(), engine.path_report()
        engine.mi_all_pairs(blocks, 20000.0, 2e5, approx)
        c1, p1 = engine.counters(), engine.path_report()
        out[key] = (engine.links(0), engine.links(1), {k: c1[k] - c0[k] for k in c1}, {k: p1[k] - p0[k] for k in p1 if k != "apx_gate"})
    engine.set_mixed(True)
    engine.set_screen(1)
    engine.set_path(0)
    assert out["verify"][2]["screen_violations"] == 0 and out["fast"][2]["screen_violations"] == 0
    assert out["fast"][3]["apx_blocks"] >= len(blocks) - 1 and out["verify"][3]["apx_blocks"] >= len(blocks) - 1, out["fast"][3]
    assert out["plain"][3]["apx_blocks"] == 0 and out["plain"][3]["plain_blocks"] >= len(blocks)
    for key in ("verify", "fast"):
        for which in (0, 1):
            for x, y in zip(out["plain"][which], out[key][which]):
                assert np.array_equal(x, y), (key, which)
    assert len(out["plain"][1][2]) > 1000
    # a gate that fails is named: 40960 sequences exceed the digit arrays' LDS budget -> limb paths, same API
    rep = engine.path_report()
    assert rep["apx_gate"].startswith("ok") and rep["pairs_listed"] > 0 and info["delta"] <= 4e-3


@pytest.mark.parametrize("Ns,weights", [(1000, "classes"), (616, "distinct"), (333, "unit")])
def test_popcount_engine_equals_mfma_engine_bit_for_bit(engine, Ns, weights):
    """LDW_ENGINE_HIST — the joint histograms on bit planes (k_cooc_popc: class-wise popcounts, three 16-bit limb sums) — produces
    the SAME exact int64 joint sums as the 5-limb MFMA GEMM, so with the shared fp64 epilogue the dense MI blocks agree bit for bit
    (diagonal, off-diagonal, ragged, N not a multiple of 32, few classes / N distinct weights / unit weights) and so do the link tables."""
    Ls = 3000
    syn = synth_alignment(Ls, Ns, seed=20 + Ns)
    st = syn["states"]
    uqe, r = orc.uqe_r(st)
    rng = np.random.default_rng(Ns)
    hdw = {"classes": lambda: 1.0 / rng.choice([1, 2, 3, 7, 31, 131, 400], Ns), "distinct": lambda: 1.0 / (rng.permutation(Ns) + 1.0),
           "unit": lambda: np.ones(Ns)}[weights]()
    d = dict(states=st, hdw=hdw, r=r, uqe=uqe, POS=syn["POS"], paint=syn["paint"], g=float(syn["g"]))
    approx = MIH.lr_links_approx(syn["POS"], float(syn["g"]), 20000.0)
    blocks = MIH.make_blocks(Ls, 1000)[:5]
    out = {}
    for kind in (L.ENGINE_MFMA, L.ENGINE_HIST):
        _setup(engine, d)
        engine.set_engine(kind)
        engine.set_mixed(False)
        engine.set_screen(0)
        engine.set_path(1)
        dense = [engine.mi_block(fi, ti) for fi, ti in ((np.arange(0, 1000), np.arange(0, 1000)), (np.arange(0, 1000), np.arange(2000, 3000)),
                                                        (np.arange(1000, 1777), np.arange(0, 1000)), (np.array([5, 9, 2999]), np.arange(40, 1077)))]
        engine.mi_all_pairs(blocks, 20000.0, 5e4, approx)
        out[kind] = (dense, engine.links(0), engine.links(1), engine.block_stats())
    engine.set_engine(L.ENGINE_MFMA)
    engine.set_mixed(True)
    engine.set_screen(1)
    engine.set_path(0)
    for x, y in zip(out[L.ENGINE_MFMA][0], out[L.ENGINE_HIST][0]):
        assert np.array_equal(x, y)
    ref = c_oracle.mi_block(st, hdw, r, uqe, np.arange(1000, 1777), np.arange(0, 1000))
    assert np.abs(out[L.ENGINE_HIST][0][2] - ref).max() < MI_TIGHT
    for which in (1, 2):
        for x, y in zip(out[L.ENGINE_MFMA][which], out[L.ENGINE_HIST][which]):
            assert np.array_equal(x, y)
    assert len(out[L.ENGINE_HIST][2][2]) > 100 and np.array_equal(out[L.ENGINE_MFMA][3]["disc_thresh"], out[L.ENGINE_HIST][3]["disc_thresh"])


def test_unsorted_positions_match_oracle(engine, synth, tmp_path):
    """snp.dat$POS in ANY order (the reference imposes none: blocks go by index, len by position, R/computePairwiseMI.R:176-177,
    :306-333).  Blocks whose lists do not ascend in POS run the plain path and the predicate-based pair list (k_gen_*): short-range
    table row-exact, long-range table row-exact up to threshold ties, thresholds and counts vs the oracle block by block — positions
    fully shuffled, and a nearly sorted order with a few swaps (so that sorted and generic blocks mix in one pass, cold and warm);
    then the drop-in entry point end to end against the oracle's a-5 loop."""
    rng = np.random.default_rng(77)
    Ls = 512
    for case in ("shuffled", "few_swaps"):
        POS = synth["POS"].copy()
        if case == "shuffled":
            POS = POS[rng.permutation(Ls)]
        else:
            for i in (40, 41, 300, 305, 470):
                POS[[i, i + 3]] = POS[[i + 3, i]]
        assert np.any(np.diff(POS.astype(np.int64)) < 0)
        d = dict(synth)
        d["POS"] = POS
        _setup(engine, d)
        g = synth["g"]
        sr_dist = 60000.0 if case == "shuffled" else 20000.0
        approx = orc.lr_links_approx(POS, g, sr_dist)
        assert MIH.lr_links_approx(POS, g, sr_dist) == approx
        blocks = np.array(orc.make_blocks(Ls, 150), dtype=np.int32)          # 4 x 4 grid, last one ragged: 10 block pairs
        for rep in range(2):
            if rep == 0:
                engine.reset_speculation()
            p0 = engine.path_report()
            engine.mi_all_pairs(blocks, sr_dist, 4000.0, approx)
            p1 = engine.path_report()
            stt = engine.block_stats()
            sr_t, lr_t = engine.links(0), engine.links(1)
            so = lo = 0
            n_generic = 0
            for bi, (fs, fe, ts, te) in enumerate(blocks.tolist()):
                fi, ti = np.arange(fs - 1, fe), np.arange(ts - 1, te)
                n_generic += bool(np.any(np.diff(POS[fi].astype(np.int64)) < 0) or np.any(np.diff(POS[ti].astype(np.int64)) < 0))
                Mb = c_oracle.mi_block(d["states"], d["hdw"], d["r"], d["uqe"], fi, ti)
                bl = orc.block_links(Mb, fi, ti, POS, d["paint"], g, sr_dist, 4000.0, approx)
                ns, nl = int(stt["n_sr"][bi]), int(stt["n_lr_kept"][bi])
                assert ns == len(bl.sr["MI"]) and int(stt["n_lr_total"][bi]) == bl.n_lr_total, (case, bi)
                assert np.array_equal(sr_t[0][so:so + ns], bl.sr["a"]) and np.array_equal(sr_t[1][so:so + ns], bl.sr["b"]), (case, bi)
                assert ns == 0 or np.abs(sr_t[2][so:so + ns] - bl.sr["MI"]).max() < MI_TIGHT
                if bl.n_lr_total:
                    assert abs(stt["disc_thresh"][bi] - bl.disc_thresh) < MI_TIGHT
                    dev = dict(zip(zip(lr_t[0][lo:lo + nl].tolist(), lr_t[1][lo:lo + nl].tolist()), lr_t[2][lo:lo + nl].tolist()))
                    ref = dict(zip(zip(bl.lr["a"].tolist(), bl.lr["b"].tolist()), bl.lr["MI"].tolist()))
                    _same_up_to_threshold_ties(ref, dev, bl.disc_thresh, MI_TIGHT)
                    # order: the rows common to both appear in the oracle's order
                    common = [k for k in zip(bl.lr["a"].tolist(), bl.lr["b"].tolist()) if k in dev]
                    assert [k for k in zip(lr_t[0][lo:lo + nl].tolist(), lr_t[1][lo:lo + nl].tolist()) if k in ref] == common
                so += ns
                lo += nl
            assert so == len(sr_t[2]) and lo == len(lr_t[2])
            assert n_generic >= (len(blocks) if case == "shuffled" else 3)
            assert p1["plain_blocks"] - p0["plain_blocks"] >= n_generic
    # the drop-in entry point on shuffled positions against the oracle's a-5 loop
    POS = synth["POS"][np.random.default_rng(3).permutation(Ls)]
    sd = SnpDat.from_states(synth["states"], POS, synth["g"])
    kw = dict(sr_dist=60000, lr_retain_links=3000, max_blk_sz=1000, srp_cutoff=0.5)
    ref = None
    for model in ("host", "device"):
        red = MIH.perform_MI_computation(sd, synth["hdw"], CdsVar(paint=synth["paint"], nclust=3), lr_save_path=str(tmp_path / f"lr_{model}.tsv"),
                                         sr_save_path=str(tmp_path / f"sr_{model}.tsv"), plt_folder=str(tmp_path / "P"), verbose=False, engine=engine,
                                         sr_model=model, **kw)
        if model == "host":
            red_host = red
    assert (tmp_path / "lr_host.tsv").read_bytes() == (tmp_path / "lr_device.tsv").read_bytes()
    assert len(red) == len(red_host)
    red = red_host
    ref = orc.perform_mi_computation(synth["states"], POS, synth["g"], sd.r, sd.uqe, synth["hdw"], synth["paint"], 3, sr_dist=60000,
                                     lr_retain_links=3000, max_blk_sz=1000, srp_cutoff=0.5)
    rr = ref.sr_links_red
    assert len(red) == len(rr["pos1"]) > 0
    ko = np.lexsort((np.asarray(rr["clust_c"]), rr["pos2"], rr["pos1"]))
    kg = np.lexsort((red["clust_c"].to_numpy(), red["pos2"].to_numpy(), red["pos1"].to_numpy()))
    for k in ("clust_c", "pos1", "pos2", "len"):
        assert np.array_equal(np.asarray(rr[k])[ko], red[k].to_numpy()[kg]), k
    assert np.abs(np.asarray(rr["MI"])[ko] - red["MI"].to_numpy()[kg]).max() < MI_TIGHT
    # the lr file: the oracle's rows; a tie group sitting on the block's threshold stays together on the device and is split in the last bit
    # by the oracle's summation order (the clonal slice is full of equal joint tables): every row the two sides disagree on has the threshold's MI
    lr_dev = pd.read_csv(tmp_path / "lr_host.tsv", sep="\t", header=None, names=["pos1", "pos2", "clust1", "clust2", "len", "MI"])
    dkeys = dict(zip(zip(lr_dev["pos1"].tolist(), lr_dev["pos2"].tolist()), lr_dev["MI"].tolist()))
    okeys = dict(zip(zip(ref.lr_rows["pos1"].astype(int).tolist(), ref.lr_rows["pos2"].astype(int).tolist()), ref.lr_rows["MI"].tolist()))
    thr = min(okeys.values())
    _same_up_to_threshold_ties(okeys, dkeys, thr, 1e-9)
    assert abs(len(dkeys) - len(okeys)) <= 0.05 * len(okeys)


def _table_digest(a, b, mi):
    """Order-sensitive 64-bit digest of a device-resident link table (wrapping int64 arithmetic): equal tables, equal digest."""
    import torch
    n = len(mi)
    if n == 0:
        return (0, 0, 0, 0)
    acc = [0, 0, 0]
    step = 1 << 27
    for lo in range(0, n, step):
        w = (torch.arange(lo, min(n, lo + step), device=mi.device, dtype=torch.int64) % 1000003) + 1
        acc[0] += int((a[lo:lo + step].long() * w).sum())
        acc[1] += int((b[lo:lo + step].long() * w).sum())
        acc[2] += int((mi[lo:lo + step].view(torch.int64) * w).sum())
    return (n,) + tuple(x & 0xFFFFFFFFFFFFFFFF for x in acc)


@pytest.mark.parametrize("Ls,N", [(100_000, 5_000), (85_000, 616), (500_000, 10_000)])
def test_full_size_properties(engine, Ls, N):
    """BASELINE config 4 at FULL size (100k SNPs x 5k sequences, 55 block pairs, the bench's workload), the shape of
    config 3 (616 genomes; the real alignment is not available offline, SURVEY 8c: synthetic of matching shape, ragged
    last block column, N not a multiple of 64) and config 5 at FULL size (500k SNPs x 10k sequences on ONE GPU: 1275 block pairs, 1.25e11
    pairs, a 2.25e9-row short-range table) through size-independent properties: every pair is accounted for exactly once, the
    long-range rows of every block are in the reference's row order and above the block's threshold, ~lr_retain_links survive,
    sampled rows of both tables equal the oracle's per-pair MI, sampled Hamming weights equal a direct count, and the default
    path (screen + approximate / mixed-precision GEMM) equals the plain one (5-limb GEMM, fp64 for every pair) bit for bit.
    Config 5 then runs the device short-range model + ARACNE on its table (invariants; a re-run is bit-identical)."""
    import torch
    big = Ls >= 500_000
    syn = synth_alignment(Ls, N, seed=1988, device="cuda", as_numpy=False)
    st_dev = syn["states"]
    engine.set_alignment(st_dev)
    cnt = engine.state_counts()
    uqe = (cnt > 0).T.astype(np.float64)
    r = uqe.sum(axis=1)
    thresh = int(Ls * 0.1)
    hdw = engine.hamming_weights(thresh)
    assert 0 < hdw.min() and hdw.max() <= 1.0
    # Hamming weights against a direct count for sampled sequences (R/performPopulationStuctureCorrection.R:23,76)
    for j in np.random.default_rng(3).integers(0, N, 6):
        diff = torch.zeros(N, dtype=torch.int64, device=st_dev.device)
        for lo in range(0, Ls, 50_000):
            diff += (st_dev[lo:lo + 50_000] != st_dev[lo:lo + 50_000, int(j)][:, None]).sum(0)
        assert hdw[j] == 1.0 / (int((diff < thresh).sum()) + 1.0), j
    engine.set_weights(hdw)
    POS, g = syn["POS"], float(syn["g"])
    engine.set_snp_meta(r, uqe, POS, syn["paint"], g)
    approx = MIH.lr_links_approx(POS, g, 20000.0)
    blocks = MIH.make_blocks(Ls, 10000)
    out = {}
    info = engine.apx_info()
    variants = dict(plain=(False, 0, 1), mixed=(True, 1, 1), fast=(True, 1, 0))   # fast = the default configuration (last: its tables stay)
    for key, (mixed, scr, path) in variants.items():
        engine.set_mixed(mixed)
        engine.set_screen(scr)
        engine.set_path(path)
        c0 = engine.counters()
        for _ in range(1 if (big and key != "fast") else 2):
            engine.mi_all_pairs(blocks, 20000.0, 1e6, approx)
        c1 = engine.counters()
        sr_t = engine.links(0, device_tensors=True)
        out[key] = (None if big else sr_t, engine.links(1), engine.block_stats(), {k: c1[k] - c0[k] for k in c1}, _table_digest(*sr_t))
        if big and key != "fast":
            del sr_t
            torch.cuda.empty_cache()
    engine.set_mixed(True)
    engine.set_screen(1)
    engine.set_path(0)
    if Ls >= 100_000:   # few weight classes (clonal groups): the default is the approximate-GEMM path
        assert info["usable"] and out["fast"][3]["apx_blocks"] >= len(blocks) and out["fast"][3]["spec_misses"] <= (2 if not big else 40)
    for key in ("mixed", "fast"):
        assert out["plain"][4] == out[key][4], key
        if not big:
            for x, y in zip(out["plain"][0], out[key][0]):
                assert torch.equal(x, y), key
        for x, y in zip(out["plain"][1], out[key][1]):
            assert np.array_equal(x, y), key
    _, (la, lb, lmi), stt, _, _ = out["fast"]
    sr = sr_t
    pairs = sum(nf * (nf - 1) // 2 if (fs, fe) == (ts, te) else nf * nt - min(nf, nt)
                for fs, fe, ts, te in blocks.tolist() for nf, nt in [(fe - fs + 1, te - ts + 1)])
    assert int(stt["n_sr"].sum() + stt["n_lr_total"].sum()) == pairs
    assert pairs == ({100_000: 4_999_500_000, 500_000: 124_987_500_000}.get(Ls) or
                     Ls * (Ls - 1) // 2 - sum(min(fe - fs, te - ts) + 1 for fs, fe, ts, te in blocks.tolist() if fs != ts))
    assert len(sr[2]) == int(stt["n_sr"].sum()) and len(lmi) == int(stt["n_lr_kept"].sum())
    assert 0.95e6 < len(lmi) < 1.05e6          # prob = 1 - lr_retain_links / lr_links_approx keeps ~1e6 in total
    off = 0
    for bi, (fs, fe, ts, te) in enumerate(blocks.tolist()):
        n = int(stt["n_lr_kept"][bi])
        a, b, m = la[off:off + n] - (fs - 1), lb[off:off + n] - (ts - 1), lmi[off:off + n]
        off += n
        assert (m >= stt["disc_thresh"][bi]).all()
        nf = fe - fs + 1
        if (fs, fe) == (ts, te):
            assert (a > b).all() and (np.diff(a.astype(np.int64) + b.astype(np.int64) * nf) > 0).all()
        else:                                    # all upper-triangle rows (a < b), then all lower ones, each column-major
            up = a < b
            k = a.astype(np.int64) + b.astype(np.int64) * nf
            nu = int(up.sum())
            assert up[:nu].all() and not up[nu:].any() and (np.diff(k[:nu]) > 0).all() and (np.diff(k[nu:]) > 0).all() and (a != b).all()
    # sampled rows against the oracle's per-pair MI with the RXY the reference reads (Q1: linear index of the nt x nf matrix)
    rng = np.random.default_rng(9)
    blk_of = lambda idx: idx // 10000
    for tab_a, tab_b, tab_m in ((la, lb, lmi), sr):
        for k in rng.integers(0, len(tab_m), 12):
            a, b, mk = int(tab_a[k]), int(tab_b[k]), float(tab_m[k])
            rows = st_dev[[a, b]].cpu().numpy()
            fa, tb = blk_of(a) * 10000, blk_of(b) * 10000
            nfb, ntb = min(10000, Ls - fa), min(10000, Ls - tb)
            rxy = orc.q1_rxy(a - fa, b - tb, nfb, ntb, r[fa:fa + nfb], r[tb:tb + ntb])
            ref = orc.mi_pair_direct(rows, hdw, r[[a, b]], uqe[[a, b]], 0, 1, rxy)
            assert abs(mk - ref) < MI_TIGHT, (a, b, mk, ref)
    if not big:
        return
    # ---- config 5: the short-range model and ARACNE on the device-resident 2.25e9-row table ----
    paint = np.asarray(syn["paint"])
    S = int(np.ceil(20000.0)) - 1
    pos_t, paint_t = torch.as_tensor(np.asarray(POS, dtype=np.int64), device=st_dev.device), torch.as_tensor(paint.astype(np.int64), device=st_dev.device)
    want = torch.zeros((3, S + 1), dtype=torch.int64, device=st_dev.device)
    n_sr = len(sr[2])
    for lo in range(0, n_sr, 1 << 27):     # counts per (cluster, len) straight from the table: sum over clusters >= n_sr
        a_, b_ = sr[0][lo:lo + (1 << 27)].long(), sr[1][lo:lo + (1 << 27)].long()
        d = (pos_t[b_] - pos_t[a_]) % int(g)
        ln = torch.minimum(d, int(g) - d)
        ok = (ln > 0) & (ln < 20000)
        for ci in (1, 2, 3):
            m = ok & ((paint_t[a_] == ci) | (paint_t[b_] == ci))
            want[ci - 1] += torch.bincount(ln[m], minlength=S + 1)[:S + 1]
        del a_, b_, d, ln, ok, m
    runs = []
    for _ in range(2):
        redd, flags, aux = srp_host.merge_n_sort_sr_links_device(engine, 3, 20000.0, 3.0, POS, paint, g, run_aracne=True)
        runs.append((redd, flags, aux))
    redd, flags, aux = runs[0]
    assert np.array_equal(aux["counts"], want[:, 1:].cpu().numpy()) and int(aux["counts"].sum()) >= n_sr
    assert set(np.unique(flags).tolist()) <= {False, True} and len(flags) == len(redd["MI"]) > 0
    assert (redd["srp_max"] > 3.0).all() and aux["n_pool"] >= len(flags)
    for k in redd:
        assert np.array_equal(redd[k], runs[1][0][k]), k
    assert np.array_equal(flags, runs[1][1])
    # the kept rows are rows of the table
    rows = torch.as_tensor(redd["row"][:1000], device=st_dev.device)
    assert np.array_equal(sr[0][rows].cpu().numpy(), redd["a"][:1000]) and np.array_equal(sr[2][rows].cpu().numpy(), redd["MI"][:1000])


def test_link_tables_regrow_mid_call(synth):
    """DevBuf::reserve_keep (ldw_alloc.cpp) under load: a FRESH context whose link tables start empty takes blocks one by one
    (ldw_mi_block_links sizes the tables per block, so the short-range and long-range tables are reallocated — and their rows
    copied — several times while earlier blocks' rows are already in them), then a larger all-pairs call after a smaller one
    (stale row counts from the previous call).  Tables must equal those of the driver that sizes the short-range table up front."""
    d = synth
    POS, g = d["POS"], d["g"]
    approx = orc.lr_links_approx(POS, g, 20000.0)
    blocks = np.array(orc.make_blocks(512, 100), dtype=np.int32)     # 15 block pairs, ascending table sizes
    with Engine(0) as ref:
        _setup(ref, d)
        ref.mi_all_pairs(blocks, 2000.0, 60000.0, approx, quirk=L.QUIRK_INTENDED)
        want = (ref.links(0), ref.links(1))
    with Engine(0) as eng:
        _setup(eng, d)
        eng.links_begin(len(blocks))
        for fs, fe, ts, te in blocks:
            eng.mi_block_links(np.arange(fs - 1, fe), np.arange(ts - 1, te), sr_dist=2000.0, lr_retain_links=60000.0, lr_links_approx=approx,
                               quirk=L.QUIRK_INTENDED)
        eng.links_end()
        got = (eng.links(0), eng.links(1))
        for w, g_ in zip(want, got):
            assert len(w[2]) > 100
            for x, y in zip(w, g_):
                assert np.array_equal(x, y)
        # a small call, then the large one in the same context: the tables grow again with the previous call's counts around
        eng.mi_all_pairs(blocks[:2], 2000.0, 60000.0, approx, quirk=L.QUIRK_INTENDED)
        small = eng.links_count(0)
        eng.mi_all_pairs(blocks, 2000.0, 60000.0, approx, quirk=L.QUIRK_INTENDED)
        assert 0 < small < eng.links_count(0)
        for w, g_ in zip(want, (eng.links(0), eng.links(1))):
            for x, y in zip(w, g_):
                assert np.array_equal(x, y)


def test_hamming_counts_strips_add_up(engine, sample, synth):
    """Sharded Hamming weights: the neighbour counts of any partition of the 128-sequence row tiles into strips
    add up to the full count, i.e. 1 / (sum + 1) is bit-identical to ldw_hamming_weights (and to the oracle)."""
    from ldweaver_amd.dist import hamming_tile_strips
    for d in (sample, synth):
        engine.set_alignment(d["states"])
        N = d["states"].shape[1]
        thr = int(d["states"].shape[0] * 0.1)
        hdw = engine.hamming_weights(thr)
        assert np.array_equal(hdw, orc.hamming_weights(d["states"], 0.1))
        ntiles = (N + 127) // 128
        for world in (1, 2, 3, 8):
            strips = hamming_tile_strips(N, world)
            assert strips[0][0] == 0 and strips[-1][1] == ntiles and all(a[1] == b[0] for a, b in zip(strips[:-1], strips[1:]))
            tot = np.zeros(N, dtype=np.int64)
            for t0, t1 in strips:
                if t1 > t0:
                    tot += engine.hamming_counts(thr, t0, t1)
            assert np.array_equal(1.0 / (tot + 1.0), hdw), world


def test_apx_path_is_exact(engine):
    """Approximate-GEMM path (ldw_set_path 2): ONE dual-digit int8 pass feeds the screen, the listed units get their exact
    joint sums from class-wise popcounts.  Those sums are the integers the 5-limb GEMM produces, so the link tables must be
    BIT-identical to the plain path (5 limbs, fp64 for every pair) — ragged last block column (Q1 scramble), both quirk
    modes, diagonal and off-diagonal blocks; verify mode evaluates every unit both ways: nothing lost by either screen."""
    syn = synth_alignment(3300, 900, seed=11)
    st = syn["states"]
    uqe, r = orc.uqe_r(st)
    engine.set_alignment(st)
    hdw = engine.hamming_weights(330)
    d = dict(states=st, hdw=hdw, r=r, uqe=uqe, POS=syn["POS"], paint=syn["paint"], g=float(syn["g"]))
    _setup(engine, d)
    info = engine.apx_info()
    assert info["usable"] and info["delta"] < 4e-3, info
    approx = MIH.lr_links_approx(syn["POS"], float(syn["g"]), 20000.0)
    blocks = MIH.make_blocks(3300, 1000)     # 1000, 1000, 1000, 300: ragged last column
    for quirk in (L.QUIRK_REFERENCE, L.QUIRK_INTENDED):
        out = {}
        for key, (scr, path, mixed) in dict(plain=(0, 1, False), apx=(1, 2, True), verify=(2, 2, True)).items():
            engine.set_mixed(mixed)
            engine.set_screen(scr)
            engine.set_path(path)
            c0 = engine.counters()
            for _ in range(2):
                engine.mi_all_pairs(blocks, 20000.0, 25000.0, approx, quirk=quirk)
            c1 = engine.counters()
            out[key] = (engine.links(0), engine.links(1), {k: c1[k] - c0[k] for k in c1})
        engine.set_mixed(True)
        engine.set_screen(1)
        engine.set_path(0)
        assert out["apx"][2]["apx_blocks"] >= len(blocks) and out["apx"][2]["mixed_blocks"] == 0
        assert out["verify"][2]["screen_violations"] == 0
        for which in (0, 1):
            for key in ("apx", "verify"):
                for x, y in zip(out["plain"][which], out[key][which]):
                    assert np.array_equal(x, y), (quirk, which, key)
        assert len(out["plain"][1][2]) > 15000 and len(out["plain"][0][2]) > 1000
        assert out["apx"][2]["apx_units_listed"] > 0 and out["apx"][2]["apx_pairs_listed"] > 0


def test_table_test_in_the_gemm_epilogue_is_verified(engine):
    """Long-range-only blocks of the approximate path: the GEMM's epilogue applies the threshold table to its own accumulators,
    neither stores the 32 x 64 regions in which every pair passes nor lets the screen look at them.  Verify mode (every
    dismissed pair is evaluated in fp64 and would count as a violation) must find nothing lost, the tables must equal the plain
    path's, and the switch must really have been on for the far off-diagonal blocks."""
    syn = synth_alignment(8400, 700, seed=23)
    poly = np.array([len(np.unique(row)) >= 2 for row in syn["states"]])    # no monomorphic SNPs: a one-row SNP's row sits at its slot index
    syn = dict(syn, states=np.ascontiguousarray(syn["states"][poly]), POS=syn["POS"][poly], paint=syn["paint"][poly])
    st = syn["states"]
    assert 7000 < len(st) <= 8400
    uqe, r = orc.uqe_r(st)
    engine.set_alignment(st)
    hdw = engine.hamming_weights(len(st) // 10)
    d = dict(states=st, hdw=hdw, r=r, uqe=uqe, POS=syn["POS"], paint=syn["paint"], g=float(syn["g"]))
    _setup(engine, d)
    assert engine.apx_info()["usable"]
    approx = MIH.lr_links_approx(syn["POS"], float(syn["g"]), 20000.0)
    blocks = MIH.make_blocks(len(st), 2000)     # 4 x 4 (or 5 x 5) grid: (1,3) and (2,4) are far apart both ways round the circular genome
    out = {}
    # ... and the tile pruning on top of it (rows ordered by minor-state weight, rare x rare wave tiles never computed): on in
    # "fast" and "verify" — whose fp64 check covers the pruned tiles' pairs like every other dismissal — off in "noprune"
    for key, (mixed, scr, path, prune) in dict(plain=(False, 0, 1, True), fast=(True, 1, 2, True), verify=(True, 2, 2, True),
                                               noprune=(True, 1, 2, False)).items():
        engine.set_mixed(mixed)
        engine.set_screen(scr)
        engine.set_path(path)
        engine.set_prune(prune)
        c0 = engine.counters()
        p0 = engine.prune_report()
        engine.gemm_stats(reset=True)
        for _ in range(2):
            engine.mi_all_pairs(blocks, 20000.0, 40000.0, approx)
        c1 = engine.counters()
        p1 = engine.prune_report()
        out[key] = (engine.links(0), engine.links(1), {k: c1[k] - c0[k] for k in c1}, engine.gemm_stats(),
                    {k: p1[k] - p0[k] for k in ("ordered_blocks", "tiles_pruned", "tiles_total")})
    engine.set_mixed(True)
    engine.set_screen(1)
    engine.set_path(0)
    engine.set_prune(True)
    assert out["fast"][3]["apx_table_launches"] >= 2 and out["verify"][3]["apx_table_launches"] >= 2, out["fast"][3]
    assert out["verify"][2]["screen_violations"] == 0
    assert out["fast"][4]["ordered_blocks"] >= 2 and out["fast"][4]["tiles_pruned"] > 0, out["fast"][4]
    assert out["verify"][4]["tiles_pruned"] > 0 and out["noprune"][4]["ordered_blocks"] == 0 and out["noprune"][4]["tiles_pruned"] == 0
    assert out["fast"][3]["apx_ops"] < out["noprune"][3]["apx_ops"]      # pruned tiles are not counted as executed work
    for which in (0, 1):
        for key in ("fast", "verify", "noprune"):
            for x, y in zip(out["plain"][which], out[key][which]):
                assert np.array_equal(x, y), (which, key)
    assert len(out["plain"][1][2]) > 10000


def test_apx_path_sr_only(engine):
    """SR-only passes need no block-wide GEMM at all in the approximate path (the screen lists the units that hold a
    short-range pair; their sums come from the popcounts): same table as the limb path, bit for bit."""
    syn = synth_alignment(2400, 800, seed=21)
    st = syn["states"]
    uqe, r = orc.uqe_r(st)
    engine.set_alignment(st)
    hdw = engine.hamming_weights(240)
    POS, g, sr_dist = syn["POS"], float(syn["g"]), 4000.0
    _setup(engine, dict(states=st, hdw=hdw, r=r, uqe=uqe, POS=POS, paint=syn["paint"], g=g))
    assert engine.apx_info()["usable"]
    blocks = orc.make_blocks(2400, 1000)
    POSf = POS.astype(float)
    res = {}
    for path in (1, 2):
        engine.set_path(path)
        c0 = engine.counters()
        engine.links_begin(len(blocks))
        for fs, fe, ts, te in blocks:
            fi, ti = np.arange(fs - 1, fe), np.arange(ts - 1, te)
            ln = np.abs(orc.circ_len(POSf[ti][None, :], POSf[fi][:, None], g))
            fi, ti = fi[(ln < sr_dist).any(axis=1)], ti[(ln < sr_dist).any(axis=0)]
            if len(fi) and len(ti):
                engine.mi_block_links(fi, ti, sr_dist=sr_dist, sr_only=True)
        engine.links_end()
        c1 = engine.counters()
        res[path] = engine.links(0)
        assert engine.links_count(1) == 0
        assert (c1["apx_blocks"] > c0["apx_blocks"]) == (path == 2)
    engine.set_path(0)
    assert len(res[1][2]) > 1000
    for x, y in zip(res[1], res[2]):
        assert np.array_equal(x, y)
    # a few rows against the oracle's per-pair MI (non-square SR-only blocks: the reference reads a scrambled RXY, so use
    # rows of the diagonal blocks, where Q1 is harmless)
    a, b, mi = res[2]
    sel = np.flatnonzero((a // 1000) == (b // 1000))[:: max(1, len(a) // 40)][:12]
    for k in sel:
        ref = orc.mi_pair_direct(st, hdw, r, uqe, int(a[k]), int(b[k]))
        assert abs(mi[k] - ref) < MI_TIGHT


def test_apx_path_on_irregular_weights(engine, synth):
    """Weights without class structure (every sequence its own value): the dual-digit approximation still holds (delta is
    bounded by the density of 7-bit x 7-bit products) and the popcount sums of the listed pairs walk one segment per
    sequence: same tables as the limb path, bit for bit.  With the screen off there is nothing to feed: forcing the path is
    refused."""
    d = dict(synth)
    rng = np.random.default_rng(3)
    d["hdw"] = rng.uniform(0.01, 1.0, len(synth["hdw"]))
    _setup(engine, d)
    info = engine.apx_info()
    assert info["usable"] and info["classes"] == len(d["hdw"]), info
    blocks = MIH.make_blocks(512, 200)
    approx = MIH.lr_links_approx(d["POS"], d["g"], 3000.0)
    res = {}
    for path in (1, 2):
        engine.set_path(path)
        c0 = engine.counters()
        for _ in range(2):
            engine.mi_all_pairs(blocks, 3000.0, 5000.0, approx)
        c1 = engine.counters()
        res[path] = (engine.links(0), engine.links(1))
        assert (c1["apx_blocks"] > c0["apx_blocks"]) == (path == 2)
    for which in (0, 1):
        for x, y in zip(res[1][which], res[2][which]):
            assert np.array_equal(x, y)
    assert len(res[1][1][2]) > 1000
    engine.set_screen(0)
    try:
        with pytest.raises(L.LdwError):
            engine.mi_all_pairs(blocks, 3000.0, 5000.0, approx)
    finally:
        engine.set_screen(1)
        engine.set_path(0)


def test_snp_bounds_hold_for_every_partner(engine):
    """The per-SNP MI bound behind the pruning of the 2 x 3 / 3 x 3 tables (k_snp_sup, ldw_snp_bounds): for an alignment full of rare
    minor states and gaps, (1) the device values equal a numpy enumeration of the vertices of the joint-table polytope, (2) NO
    pair of the alignment — every partner the oracle can offer, both readings of RXY (quirk Q1 on a square and on a ragged
    block) — has an MI above the bound of either SNP for the other's kind, and (3) the bound is tight: a partner built to sit
    on the best vertex reaches it to 1e-9."""
    import itertools
    rng = np.random.default_rng(5)
    Ls, N = 700, 420
    st = np.zeros((Ls, N), dtype=np.uint8)
    for a in range(Ls):
        maj, mnr = rng.choice(4, size=2, replace=False)
        nm = int(rng.choice([1, 1, 2, 3, 5, 9, 30, 120]))
        st[a] = maj
        st[a, rng.choice(N, nm, replace=False)] = mnr
        if a % 4 == 0:                                                   # a third state: gaps
            st[a, rng.choice(N, int(rng.choice([1, 2, 6, 40])), replace=False)] = 4
        if a % 7 == 3:                                                   # strong LD with the previous SNP
            st[a] = np.where(st[a - 1] == st[a - 1][0], maj, mnr)
    uqe, r = orc.uqe_r(st)
    hdw = 1.0 / rng.integers(1, 6, size=N).astype(np.float64)
    POS = np.sort(rng.choice(np.arange(1, 300000), size=Ls, replace=False)).astype(np.int32)
    d = dict(states=st, hdw=hdw, r=r, uqe=uqe, POS=POS, paint=np.ones(Ls, np.int32), g=300000.0)
    _setup(engine, d)
    sup = engine.snp_bounds()                                            # [snp, RXY reading, partner kind - 2]
    kind = np.where((r == 2) | (r == 3), r, 0).astype(int)               # (uqe_r flags exactly the states that are present)
    assert (kind == 2).sum() > 300 and (kind == 3).sum() > 100
    v = np.sqrt(hdw) ** 2
    neff = float(hdw.sum())
    rmin = float(r.min())

    def vertex_sup(p, kb, rxy):
        ka = len(p)
        den = neff + 0.5 * ka * kb
        best = -1e300
        for phi in itertools.product(range(kb), repeat=ka):
            n = np.zeros((ka, kb))
            for x, y in enumerate(phi):
                n[x, y] = p[x]
            pY = n.sum(0)
            D = np.outer(p, pY) + rxy + (p * 0.5 * ka)[:, None] + (pY * 0.5 * kb)[None, :]
            best = max(best, float(((n + 0.5) * np.log((n + 0.5) * den / D)).sum() / den))
        return best

    checked = 0
    for a in rng.choice(np.where(kind > 0)[0], 60, replace=False):
        p = np.array([v[st[a] == x].sum() for x in range(5) if (st[a] == x).any()])
        if sup[a, 0, 0] > 1e299:
            continue                                                     # sizeable minor state: not evaluated by design
        for kb in (2, 3):
            ka = int(kind[a])
            assert abs(sup[a, 0, kb - 2] - vertex_sup(p, kb, 0.25 * ka * kb)) < 1e-9
            assert abs(sup[a, 1, kb - 2] - vertex_sup(p, kb, min(0.25 * ka * kb, 0.25 * rmin * rmin))) < 1e-9
        checked += 1
    assert checked > 30
    # (2) every pair of the alignment, three readings of RXY
    blocks = [(np.arange(0, 350), np.arange(350, 700), L.QUIRK_INTENDED, 0), (np.arange(0, 350), np.arange(350, 700), L.QUIRK_REFERENCE, 1),
              (np.arange(0, 400), np.arange(400, 700), L.QUIRK_REFERENCE, 1), (np.arange(0, 350), np.arange(0, 350), L.QUIRK_REFERENCE, 1)]
    n_bound = 0
    for fi, ti, quirk, m in blocks:
        M = engine.mi_block(fi, ti, quirk=quirk)
        ka, kb = kind[fi][:, None], kind[ti][None, :]
        ok = (ka > 0) & (kb > 0) & (fi[:, None] != ti[None, :])
        ba = np.where(kb == 3, sup[fi, m, 1][:, None], sup[fi, m, 0][:, None])      # a's bound against b's kind
        bb = np.where(ka == 3, sup[ti, m, 1][None, :], sup[ti, m, 0][None, :])
        assert np.all(M[ok] <= ba[ok] + 1e-12) and np.all(M[ok] <= bb[ok] + 1e-12), (quirk, float((M - ba)[ok].max()), float((M - bb)[ok].max()))
        n_bound += int(((ba < 1e299) & ok).sum())
    assert n_bound > 100000
    # (3) tightness: copy a rare SNP into a partner with the same split (the vertex "minor -> minor, major -> major")
    a = int(np.where((kind == 2) & (sup[:, 0, 0] < 1e299))[0][0])
    st2 = st.copy()
    b = a + 1 if a + 1 < Ls else a - 1
    vals = [x for x in range(5) if (st[a] == x).any()]
    st2[b] = np.where(st[a] == vals[0], 0, 1)
    uqe2, r2 = orc.uqe_r(st2)
    _setup(engine, dict(d, states=st2, uqe=uqe2, r=r2))
    sup2 = engine.snp_bounds()
    M = engine.mi_block(np.array([a]), np.array([b]), quirk=L.QUIRK_INTENDED)
    assert abs(M[0, 0] - sup2[a, 0, 0]) < 1e-9 and M[0, 0] <= sup2[a, 0, 0] + 1e-12


def test_bad_block_in_the_middle_of_a_pass_is_reported_and_the_engine_survives(engine, synth):
    """The block lists are prepared by a helper thread that runs ahead of the submitting thread: an invalid block in the middle of a pass
    must come back as an ordinary error — no hang, no crash, the message of the helper's check — and the next pass on the same context
    must give the usual tables."""
    d = synth
    _setup(engine, d)
    Ls = len(d["states"])
    approx = orc.lr_links_approx(d["POS"], d["g"], 20000.0)
    blocks = np.array(orc.make_blocks(Ls, max(64, Ls // 6)), dtype=np.int32)
    assert len(blocks) >= 10
    engine.mi_all_pairs(blocks, 20000.0, 5000.0, approx)
    ref = (engine.links(0), engine.links(1))
    bad = blocks.copy()
    bad[len(bad) // 2, 1] = Ls + 5                                      # from-range runs past the alignment
    with pytest.raises(L.LdwError) as ei:
        engine.mi_all_pairs(bad, 20000.0, 5000.0, approx)
    assert "outside 1.." in str(ei.value)
    for _ in range(2):
        engine.mi_all_pairs(blocks, 20000.0, 5000.0, approx)
        for which in (0, 1):
            for x, y in zip(ref[which], engine.links(which)):
                assert np.array_equal(x, y)


def test_pruning_under_the_reference_rxy_with_monomorphic_snps(engine):
    """Quirk Q1 reads RXY from two OTHER SNPs of the block; with monomorphic SNPs in it (r = 1) the scrambled RXY can fall to 1/4, below
    the RXY = 1 the biallelic threshold table is built for and below the proper RXY of the per-SNP bounds.  The table must then stay
    off and the bounds must use the floor r_min^2 / 4: default path (pruning on) == plain path, verify mode finds nothing lost, on an
    alignment with rare states, gaps and monomorphic sites, ragged last block column."""
    rng = np.random.default_rng(91)
    Ls, N = 2400, 512
    st = np.zeros((Ls, N), dtype=np.uint8)
    for a in range(Ls):
        maj, mnr = rng.choice(4, size=2, replace=False)
        st[a] = maj
        if a % 9 != 4:                                                   # (a % 9 == 4: monomorphic, r = 1)
            st[a, rng.choice(N, int(rng.choice([1, 1, 2, 3, 8, 40, 150])), replace=False)] = mnr
        if a % 5 == 0:
            st[a, rng.choice(N, int(rng.choice([1, 3, 20])), replace=False)] = 4
        if a % 11 == 7 and a > 0:
            st[a] = np.where(st[a - 1] == st[a - 1][0], maj, mnr)
    uqe, r = orc.uqe_r(st)
    assert r.min() == 1
    POS = np.sort(rng.choice(np.arange(1, 400000), size=Ls, replace=False)).astype(np.int32)
    hdw = 1.0 / rng.integers(1, 5, size=N).astype(np.float64)
    d = dict(states=st, hdw=hdw, r=r, uqe=uqe, POS=POS, paint=rng.integers(1, 4, Ls).astype(np.int32), g=400000.0)
    _setup(engine, d)
    assert engine.apx_info()["usable"]
    approx = orc.lr_links_approx(POS, d["g"], 20000.0)
    blocks = np.array(orc.make_blocks(Ls, 1000), dtype=np.int32)       # 1000, 1000, 400
    out = {}
    for key, (mixed, scr, path) in dict(plain=(False, 0, 1), apx=(True, 1, 2), verify=(True, 2, 2)).items():
        engine.set_mixed(mixed)
        engine.set_screen(scr)
        engine.set_path(path)
        c0, p0 = engine.counters(), engine.prune_report()
        for _ in range(2):
            engine.mi_all_pairs(blocks, 20000.0, 20000.0, approx, quirk=L.QUIRK_REFERENCE)
        c1, p1 = engine.counters(), engine.prune_report()
        out[key] = (engine.links(0), engine.links(1), {k: c1[k] - c0[k] for k in c1}, p1["tiles_pruned"] - p0["tiles_pruned"])
    engine.set_mixed(True)
    engine.set_screen(1)
    engine.set_path(0)
    assert out["verify"][2]["screen_violations"] == 0 and out["apx"][2]["apx_blocks"] >= len(blocks)
    for which in (0, 1):
        for key in ("apx", "verify"):
            for x, y in zip(out["plain"][which], out[key][which]):
                assert np.array_equal(x, y), (which, key)
    assert len(out["plain"][1][2]) > 5000
    # the bounds carry the floor: with r_min = 1 the reference-mode values sit above the intended-mode ones
    sup = engine.snp_bounds()
    fin = sup[:, 0, 0] < 1e299
    assert fin.sum() > 500 and np.all(sup[fin, 1, :] >= sup[fin, 0, :] - 1e-15) and np.any(sup[fin, 1, 0] > sup[fin, 0, 0] + 1e-6)


def test_spans_equal_block_by_block(engine):
    """r04 spans: consecutive long-range-only block pairs of one block row run as ONE launch sequence over their concatenated to side
    (VERDICT r03 item 1), every reference block keeping its own histogram, threshold, candidate list, row order and place in the append
    order (R/computePairwiseMI.R:103-116, :352-362).  40k SNPs x 2k sequences, 8 x 8 blocks of 5000 (36 block pairs; rows of up to five
    long-range-only pairs), cold and warm passes, both readings of RXY: link tables, per-block thresholds and row counts with spans ==
    without == the plain path (5-limb GEMM, fp64 MI of every pair) bit for bit; then the overflow fallback: pair lists forced to 64
    entries make every segment of every span (and every lone block) fall back like a wrong guess — redone on its own, non-speculatively,
    in its place in the order — tables still identical."""
    Ls, N, B = 40_000, 2_000, 5_000
    syn = synth_alignment(Ls, N, seed=1988, device="cuda", as_numpy=False)
    engine.set_engine(L.ENGINE_MFMA)
    engine.set_alignment(syn["states"])
    cnt = engine.state_counts()
    uqe = (cnt > 0).T.astype(np.float64)
    r = uqe.sum(axis=1)
    hdw = engine.hamming_weights(int(Ls * 0.1))
    engine.set_weights(hdw)
    POS, g = syn["POS"], float(syn["g"])
    engine.set_snp_meta(r, uqe, POS, syn["paint"], g)
    approx = MIH.lr_links_approx(POS, g, 20000.0)
    blocks = MIH.make_blocks(Ls, B)
    assert len(blocks) == 36

    def run(quirk, cold):
        if cold:
            engine.reset_speculation()
        engine.mi_all_pairs(blocks, 20000.0, 1e6, approx, quirk=quirk)
        return engine.links(0), engine.links(1), engine.block_stats()

    def same(x, y, what):
        for which in (0, 1):
            for a, b in zip(x[which], y[which]):
                assert np.array_equal(a, b), (what, which)
        for k in ("n_lr_total", "n_lr_kept", "n_sr", "disc_thresh"):
            assert np.array_equal(x[2][k], y[2][k]), (what, k)

    try:
        for quirk in (L.QUIRK_REFERENCE, L.QUIRK_INTENDED):
            engine.set_mixed(False)
            engine.set_screen(0)
            engine.set_path(1)
            plain = run(quirk, True)
            engine.set_mixed(True)
            engine.set_screen(1)
            engine.set_path(0)
            engine.set_span(False)
            off_cold = run(quirk, True)
            off_warm = run(quirk, False)
            engine.set_span(True)
            s0 = engine.span_report()
            on_cold = run(quirk, True)
            on_warm = run(quirk, False)
            s1 = engine.span_report()
            assert s1["spans"] - s0["spans"] >= 8 and s1["blocks"] - s0["blocks"] >= 24, (s0, s1)   # (rows 0..4 hold 5, 5, 4, 3, 2 long-range-only pairs; twice)
            for tag, t in (("off cold", off_cold), ("off warm", off_warm), ("on cold", on_cold), ("on warm", on_warm)):
                same(plain, t, (quirk, tag))
            assert len(plain[1][2]) > 500_000 and len(plain[0][2]) > 1_000_000
            # the index columns of the short-range table from the positions alone (ldw_sr_pairs_fill: what rank 0 of a multi-GPU run rebuilds
            # instead of receiving) == the pass's own
            pa, pb = engine.sr_pairs(blocks, 20000.0)
            assert np.array_equal(pa.cpu().numpy(), plain[0][0]) and np.array_equal(pb.cpu().numpy(), plain[0][1])
            # shorter spans give the same tables
            engine.set_span(True, 2)
            same(plain, run(quirk, True), (quirk, "spans of 2"))
            with pytest.raises(L.LdwError) as ei:   # (corner spans were measured slower and removed)
                engine.set_span(True, 8, corners=True)
            assert ei.value.code == L.LDW_ERR_STATE
            engine.set_span(True, 8)
        # r04 (end): the queue assignment of long alignments — screens at the head of phase 2 on the main stream, exact band GEMM on the GEMM
        # stream, every item keeping the threshold table of its first phase — forced on this short one, through the same variants
        import os
        os.environ["LDW_QUEUE_SWAP_KW"] = "1"
        try:
            for quirk in (L.QUIRK_REFERENCE, L.QUIRK_INTENDED):
                engine.set_mixed(False); engine.set_screen(0); engine.set_path(1)
                plain_q = run(quirk, True)
                engine.set_mixed(True); engine.set_screen(1); engine.set_path(0)
                engine.set_span(True, 8)
                same(plain_q, run(quirk, True), (quirk, "queues swapped, spans, cold"))
                same(plain_q, run(quirk, False), (quirk, "queues swapped, spans, warm"))
                engine.set_span(False, 8)
                same(plain_q, run(quirk, True), (quirk, "queues swapped, no spans"))
                engine.set_span(True, 8)
        finally:
            os.environ.pop("LDW_QUEUE_SWAP_KW")
        # overflow: every pair list holds 64 entries -> every speculative block / segment is redone non-speculatively
        Engine.set_pair_cap(64)
        c0, s0 = engine.counters(), engine.span_report()
        over = run(L.QUIRK_REFERENCE, True)
        c1, s1 = engine.counters(), engine.span_report()
        Engine.set_pair_cap(0)
        assert s1["redone"] - s0["redone"] >= 10 and c1["spec_misses"] - c0["spec_misses"] >= 20, (s0, s1, c0, c1)
        # r04, the maybe list (entries outside their table thresholds, handed over by the GEMM's epilogue): the same tables without it, and a
        # list of 16 entries overflows -> its block takes the pair lists' overflow path
        import os
        os.environ["LDW_NO_MAYBE"] = "1"
        try:
            no_maybe = run(L.QUIRK_REFERENCE, True)
        finally:
            os.environ.pop("LDW_NO_MAYBE")
        os.environ["LDW_MAYBE_CAP"] = "16"
        try:
            c0, o0 = engine.counters(), engine.overflow_report()
            tiny = run(L.QUIRK_REFERENCE, True)
            c1, o1 = engine.counters(), engine.overflow_report()
        finally:
            os.environ.pop("LDW_MAYBE_CAP")
        # r05: the first overflow switches the list off for the rest of the pass — only the items already in flight (3 pipeline slots) are redone,
        # not block after block as in r04; the next cold pass (ldw_reset_speculation) starts with the list on again
        n_over = o1["maybe_list"] - o0["maybe_list"]
        assert n_over >= 1 and o1["maybe_off"], (o0, o1)
        assert c1["spec_misses"] - c0["spec_misses"] >= n_over, (c0, c1)
        assert n_over <= 3 * 8, (o0, o1)
        engine.reset_speculation()
        assert not engine.overflow_report()["maybe_off"]
        engine.set_mixed(False)
        engine.set_screen(0)
        engine.set_path(1)
        plain_ref = run(L.QUIRK_REFERENCE, True)
        same(plain_ref, over, "pair-list overflow")
        same(plain_ref, no_maybe, "without the maybe list")
        same(plain_ref, tiny, "maybe-list overflow")
    finally:
        Engine.set_pair_cap(0)
        engine.set_span(True, 8)
        engine.set_mixed(True)
        engine.set_screen(1)
        engine.set_path(0)


@pytest.mark.parametrize("weights", ["hamming", "distinct"])
def test_adversarial_alignment_default_equals_plain(engine, weights):
    """data that is NOT friendly to the default path — MAF uniform in [0.2, 0.5] (no rare minor states: the
    marginal-only tile pruning has nothing to dismiss), no clonal groups (synth kind 'adversarial') — 20k SNPs x 2k sequences, 5000-SNP
    blocks; with the weights estimate_Hamming_distance_weights gives there (all equal) and with N DISTINCT weights (per-k-step block
    exponents).  The default path's tables == the plain path's bit for bit, cold and warm; verify mode (every pair evaluated both ways,
    block by block and screen dismissals checked in fp64): 0 violations."""
    Ls, N, B = 20_000, 2_000, 5_000
    syn = synth_alignment(Ls, N, seed=1988, device="cuda", as_numpy=False, kind="adversarial")
    engine.set_engine(L.ENGINE_MFMA)
    engine.set_alignment(syn["states"])
    cnt = engine.state_counts()
    uqe = (cnt > 0).T.astype(np.float64)
    r = uqe.sum(axis=1)
    hdw = engine.hamming_weights(int(Ls * 0.1))
    if weights == "hamming":
        assert len(np.unique(hdw)) <= 3          # no sequence has a neighbour within 10 %: (nearly) all weights equal
    else:
        u = ((np.arange(N, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 32)).astype(np.float64) / float(1 << 32)
        hdw = 1.0 / (1.0 + 49.0 * u)
        assert len(np.unique(hdw)) == N
    engine.set_weights(hdw)
    POS, g = syn["POS"], float(syn["g"])
    engine.set_snp_meta(r, uqe, POS, syn["paint"], g)
    approx = MIH.lr_links_approx(POS, g, 20000.0)
    blocks = MIH.make_blocks(Ls, B)
    lr_retain = 2e5     # keeps 0.1 % of the 2e8 pairs: the speculative path is the automatic choice
    out = {}
    try:
        # (classwise: r05 — the exact sums of the listed pairs by the class-wise popcount kernel where the default walks the set bits against a
        # per-position weight table, k_pair_sums_bits: the form weightings with many classes take; same integers, so the same tables)
        for key, (mixed, scr, path, cold) in dict(plain=(False, 0, 1, True), cold=(True, 1, 0, True), warm=(True, 1, 0, False), verify=(True, 2, 0, False),
                                                  classwise=(True, 1, 0, False)).items():
            engine.set_mixed(mixed)
            engine.set_screen(scr)
            engine.set_path(path)
            if key == "classwise":
                os.environ["LDW_NO_PAIR_BITS"] = "1"
            else:
                os.environ.pop("LDW_NO_PAIR_BITS", None)
            if cold:
                engine.reset_speculation()
            c0, o0, s0 = engine.counters(), engine.overflow_report(), engine.span_report()
            engine.mi_all_pairs(blocks, 20000.0, lr_retain, approx)
            c1, o1, s1 = engine.counters(), engine.overflow_report(), engine.span_report()
            d = {k: c1[k] - c0[k] for k in c1}
            d.update(pair_list_overflows=o1["pair_list"] - o0["pair_list"], maybe_list_overflows=o1["maybe_list"] - o0["maybe_list"],
                     span_blocks_redone=s1["redone"] - s0["redone"], maybe_off=o1["maybe_off"])
            out[key] = (engine.links(0), engine.links(1), engine.block_stats(), d)
    finally:
        os.environ.pop("LDW_NO_PAIR_BITS", None)
        engine.set_mixed(True)
        engine.set_screen(1)
        engine.set_path(0)
    info, rep = engine.apx_info(), engine.path_report()
    assert info["usable"], (info, rep)
    assert out["warm"][3]["apx_blocks"] == len(blocks) and out["verify"][3]["screen_violations"] == 0 and out["cold"][3]["screen_violations"] == 0
    # r05: equal tables are not enough — r04's maybe list overflowed on exactly this data, every block was redone on the
    # plain path and the tables still came out right.  No block may be redone, cold or warm, and no list may overflow.
    for key in ("cold", "warm"):
        d = out[key][3]
        assert d["spec_misses"] == 0 and d["span_blocks_redone"] == 0, (key, d)
        assert d["pair_list_overflows"] == 0 and d["maybe_list_overflows"] == 0 and not d["maybe_off"], (key, d)
        assert d["apx_blocks"] >= len(blocks) - 1, (key, d)   # (cold: the pass's very first block may run before its kind has a guess)
    for key in ("cold", "warm", "verify", "classwise"):
        for which in (0, 1):
            for x, y in zip(out["plain"][which], out[key][which]):
                assert np.array_equal(x, y), (key, which)
        for k in ("n_lr_total", "n_lr_kept", "n_sr", "disc_thresh"):
            assert np.array_equal(out["plain"][2][k], out[key][2][k]), (key, k)
    assert len(out["plain"][1][2]) > 100_000 and len(out["plain"][0][2]) > 100_000


def _pin_selection_of_blocks(engine, st_dev, hdw, r, uqe, POS, g, approx, sub, whole_with_c_oracle=()):
    """For each block of `sub`: dense device MI (ldw_mi_block, reference quirk mode) against the oracle — a 512 x 512 sub-block through
    c_oracle in intended mode + 16 single pairs with the block's own Q1 geometry, or (block index in whole_with_c_oracle) the WHOLE block
    against c_oracle.mi_block in reference quirk mode — then the oracle's selection rule on the dense MI against the default path's rows,
    MI bits and threshold, cold and warm.  Returns per-block (n_lr, n_kept)."""
    import torch
    want = []
    for bi, (fs, fe, ts, te) in enumerate(sub.tolist()):
        fi, ti = np.arange(fs - 1, fe), np.arange(ts - 1, te)
        diag = (fs, fe) == (ts, te)
        Md = engine.mi_block(fi, ti)
        if bi in whole_with_c_oracle:
            rows_needed = np.unique(np.concatenate([fi, ti]))
            st_sub = st_dev[torch.as_tensor(rows_needed, device=st_dev.device)].cpu().numpy()
            Mo = c_oracle.mi_block(st_sub, hdw, r[rows_needed], uqe[rows_needed], np.searchsorted(rows_needed, fi), np.searchsorted(rows_needed, ti))
            assert Mo.shape == Md.shape
            err = float(np.abs(Md - Mo).max())
            assert err < MI_TIGHT, (bi, err)
            del Mo, st_sub
        else:
            Mi = engine.mi_block(fi, ti, quirk=L.QUIRK_INTENDED)
            o_f, o_t = min(3000, len(fi) - 512), min(3000 if diag else 6100, len(ti) - 512)
            sf, stt_ = fi[o_f:o_f + 512], ti[o_t:o_t + 512]
            rows_needed = np.unique(np.concatenate([sf, stt_]))
            st_sub = st_dev[torch.as_tensor(rows_needed, device=st_dev.device)].cpu().numpy()
            loc_f, loc_t = np.searchsorted(rows_needed, sf), np.searchsorted(rows_needed, stt_)
            allr = np.arange(len(rows_needed))
            Mo = c_oracle.mi_block(st_sub, hdw, r[rows_needed], uqe[rows_needed], allr, allr)
            assert np.abs(Mi[o_f:o_f + 512, o_t:o_t + 512] - Mo[np.ix_(loc_f, loc_t)]).max() < MI_TIGHT
            rng = np.random.default_rng(31 + bi)
            for _ in range(16):
                a_l, b_l = int(rng.integers(0, len(fi))), int(rng.integers(0, len(ti)))
                rows2 = st_dev[[int(fi[a_l]), int(ti[b_l])]].cpu().numpy()
                rxy = orc.q1_rxy(a_l, b_l, len(fi), len(ti), r[fi], r[ti])
                refv = orc.mi_pair_direct(rows2, hdw, r[[fi[a_l], ti[b_l]]], uqe[[fi[a_l], ti[b_l]]], 0, 1, rxy)
                assert abs(Md[a_l, b_l] - refv) < MI_TIGHT
            del Mi
        want.append(_dense_block_selection(Md, fi, ti, POS, g, 20000.0, 1e6, approx, diag))
        del Md
    for cold in (True, False):
        if cold:
            engine.reset_speculation()
        c0 = engine.counters()
        engine.mi_all_pairs(sub, 20000.0, 1e6, approx)
        c1 = engine.counters()
        assert c1["apx_blocks"] - c0["apx_blocks"] >= (1 if cold else len(sub)), (cold, c0, c1)       # the default path, not a fallback
        stt = engine.block_stats()
        la, lb, lmi = engine.links(1)
        off = 0
        for bi, (wa, wb, wmi, thr, n_lr) in enumerate(want):
            n = int(stt["n_lr_kept"][bi])
            assert int(stt["n_lr_total"][bi]) == n_lr
            assert stt["disc_thresh"][bi] == thr, (bi, cold, stt["disc_thresh"][bi], thr)
            assert n == len(wmi), (bi, cold, n, len(wmi))
            assert np.array_equal(la[off:off + n], wa) and np.array_equal(lb[off:off + n], wb), (bi, cold)
            assert np.array_equal(lmi[off:off + n], wmi), (bi, cold)
            off += n
        assert off == len(lmi)
    return [(w[4], len(w[2])) for w in want]


def test_c5_blocks_selection_pinned_to_oracle(engine):
    """VERDICT r03 item 3a, first half: the C4 treatment (test_c4_blocks_selection_pinned_to_oracle) at BASELINE config 5's size —
    500k SNPs x 10k sequences (N = 10 000: twice the K of C4, 100 weight-class segments more), one DIAGONAL and one OFF-DIAGONAL
    10k x 10k block pair from the middle of the 1275: dense device MI against the C oracle (512 x 512 sub-block + the block's own Q1
    geometry per pair), then the oracle's selection rule on the dense MI == the default path's rows, MI bits and threshold, cold and warm."""
    Ls, N = 500_000, 10_000
    syn = synth_alignment(Ls, N, seed=1988, device="cuda", as_numpy=False)
    st_dev = syn["states"]
    engine.set_alignment(st_dev)
    cnt = engine.state_counts()
    uqe = (cnt > 0).T.astype(np.float64)
    r = uqe.sum(axis=1)
    hdw = engine.hamming_weights(int(Ls * 0.1))
    engine.set_weights(hdw)
    POS, g = syn["POS"], float(syn["g"])
    engine.set_snp_meta(r, uqe, POS, syn["paint"], g)
    approx = MIH.lr_links_approx(POS, g, 20000.0)
    blocks = MIH.make_blocks(Ls, 10000)
    assert len(blocks) == 1275
    i_diag = next(i for i, b in enumerate(blocks.tolist()) if b[0] == b[2] and b[0] == 200_001)
    i_off = next(i for i, b in enumerate(blocks.tolist()) if b[0] == 200_001 and b[2] == 350_001)
    res = _pin_selection_of_blocks(engine, st_dev, hdw, r, uqe, POS, g, approx, blocks[[i_diag, i_off]])
    assert res[0][0] < res[1][0] == 10_000 * 10_000 - 10_000 and all(n_lr > 1e7 and 50 < kept < 5000 for n_lr, kept in res), res   # (4.4 bp per SNP: most of a diagonal block's pairs are short-range)


def test_ragged_block_whole_against_c_oracle(engine):
    """VERDICT r03 item 3a, second half: the shape of BASELINE config 3 (85 000 SNPs x 616 sequences: the last block column is 5000 wide,
    N is no multiple of 64, 616 sequences in few clonal groups) — one RAGGED 10 000 x 5 000 block compared WHOLE (5e7 pairs) with
    c_oracle.mi_block in the reference's quirk mode: the only geometry where Q1 scrambles RXY (rft = t(rf rt') read by the linear index
    of the nf x nt matrix: R/computePairwiseMI.R:261 against src/computeMI.cpp:19) instead of merely transposing it — plus a square
    off-diagonal neighbour of the same row through the sampled treatment; then the oracle's selection rule on the dense device MI ==
    the default path's rows, MI bits and thresholds, cold and warm."""
    Ls, N = 85_000, 616
    syn = synth_alignment(Ls, N, seed=1988, device="cuda", as_numpy=False)
    st_dev = syn["states"]
    engine.set_alignment(st_dev)
    cnt = engine.state_counts()
    uqe = (cnt > 0).T.astype(np.float64)
    r = uqe.sum(axis=1)
    hdw = engine.hamming_weights(int(Ls * 0.1))
    engine.set_weights(hdw)
    POS, g = syn["POS"], float(syn["g"])
    engine.set_snp_meta(r, uqe, POS, syn["paint"], g)
    approx = MIH.lr_links_approx(POS, g, 20000.0)
    blocks = MIH.make_blocks(Ls, 10000)
    bl = blocks.tolist()
    i_rag = next(i for i, b in enumerate(bl) if b[0] == 30_001 and b[2] == 80_001)
    i_sq = next(i for i, b in enumerate(bl) if b[0] == 30_001 and b[2] == 60_001)
    assert bl[i_rag] == [30_001, 40_000, 80_001, 85_000]
    res = _pin_selection_of_blocks(engine, st_dev, hdw, r, uqe, POS, g, approx, blocks[[i_sq, i_rag]], whole_with_c_oracle=(1,))
    assert res[1][0] == 10_000 * 5_000 - 5_000 and all(kept > 1000 for _, kept in res), res


@pytest.mark.parametrize("case", ["npad_gate", "many_classes"])
def test_gates_of_the_approximate_path_fall_back_to_the_limb_paths(engine, case):
    """the gates of the approximate path that no test reached (prepare_apx_weights, ldw_apx.hip).  (i) more than
    30 720 padded sequences — the two digit arrays no longer fit the GEMM's LDS beside its tables: N = 30 848: ldw_path_report names the
    gate, the blocks run the limb paths (mixed precision: 3 high limbs + gathered low limbs) with the screen.  (ii) r03's third gate —
    so many weight classes that the popcount segment tables of k_pair_sums exceed 60 000 bytes of LDS: 4000 DISTINCT weights — is GONE:
    the approximate path runs, and its pair sums walk the set bits against a per-position weight table in 32 KB of LDS (k_pair_sums_bits;
    the class-wise form with global tables is reached above Npad 20 480 or with LDW_NO_PAIR_BITS: tests/test_sequence_count_edges.py).  Either way the link tables equal the plain
    path's bit for bit.  (The remaining fallback — a pair list that overflows — is forced in test_spans_equal_block_by_block with
    ldw_set_pair_cap.)"""
    if case == "npad_gate":
        Ls, N = 2_400, 30_848
    else:
        Ls, N = 2_400, 4_000
    syn = synth_alignment(Ls, N, seed=5, device="cuda", as_numpy=False)
    engine.set_engine(L.ENGINE_MFMA)
    engine.set_alignment(syn["states"])
    cnt = engine.state_counts()
    uqe = (cnt > 0).T.astype(np.float64)
    r = uqe.sum(axis=1)
    hdw = engine.hamming_weights(int(Ls * 0.1))
    if case == "many_classes":
        u = ((np.arange(N, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 32)).astype(np.float64) / float(1 << 32)
        hdw = 1.0 / (1.0 + 49.0 * u)
    engine.set_weights(hdw)
    POS, g = syn["POS"], float(syn["g"])
    engine.set_snp_meta(r, uqe, POS, syn["paint"], g)
    info, rep = engine.apx_info(), engine.path_report()
    if case == "npad_gate":
        assert not info["usable"] and "Npad" in rep["apx_gate"] and "30720" in rep["apx_gate"], (info, rep)
    else:
        assert info["usable"] and info["classes"] == N and info["segments"] * 16 > 60000 and info["delta"] <= 4e-3, (rep, info)
    approx = MIH.lr_links_approx(POS, g, 20000.0)
    blocks = MIH.make_blocks(Ls, 1200)
    lr_retain = 4000.0    # 0.14 % of the 2.9e6 pairs: speculation is the automatic choice
    out = {}
    try:
        for key, (mixed, scr, path) in dict(plain=(False, 0, 1), default=(True, 1, 0), verify=(True, 2, 0)).items():
            engine.set_mixed(mixed)
            engine.set_screen(scr)
            engine.set_path(path)
            if key != "verify":
                engine.reset_speculation()
            c0, f0 = engine.counters(), engine.form_report()
            for _ in range(2):
                engine.mi_all_pairs(blocks, 20000.0, lr_retain, approx)
            c1, f1 = engine.counters(), engine.form_report()
            out[key] = (engine.links(0), engine.links(1), engine.block_stats(), {k: c1[k] - c0[k] for k in c1}, {k: f1[k] - f0[k] for k in f1})
    finally:
        engine.set_mixed(True)
        engine.set_screen(1)
        engine.set_path(0)
    d = out["default"][3]
    if case == "npad_gate":
        assert d["apx_blocks"] == 0 and d["mixed_blocks"] >= len(blocks), d     # the gate sent every speculative block to the limb paths
    else:
        assert d["apx_blocks"] >= len(blocks) and d["apx_pairs_listed"] > 0, d   # ... and here the approximate path ran, its pair sums by the bit walk
        f = out["default"][4]
        assert f["bits_lds64"] > 0 and f["bits_lds160"] == f["classwise_lds"] == f["classwise_global"] == 0, f
    assert out["verify"][3]["screen_violations"] == 0
    for key in ("default", "verify"):
        for which in (0, 1):
            for x, y in zip(out["plain"][which], out[key][which]):
                assert np.array_equal(x, y), (case, key, which)
        for k in ("n_lr_total", "n_lr_kept", "n_sr", "disc_thresh"):
            assert np.array_equal(out["plain"][2][k], out[key][2][k]), (case, key, k)
    assert len(out["plain"][1][2]) > 1000


def test_in_process_multi_context_equals_one_context(sample, tmp_path):
    """VERDICT r04 item 3 / SURVEY 8(b)(5): ldw_mi_all_pairs_multi — the block loop of R/computePairwiseMI.R:103-116 dealt over several
    contexts of ONE process (worker threads inside the library, peer-to-peer gather into ctx[0]) — with TWO and THREE contexts on this
    box's one GPU: link tables, block statistics and lr_links.tsv bytes identical to one context; the short-range rows travel with their
    MI column alone (default: index columns rebuilt by ldw_sr_pairs_fill on the device) or with their index columns (LDW_MULTI_SR_FULL_ROWS); unsorted positions and
    an SR-only parameter set; the Hamming weights shared over the contexts are bit-identical; a context
    with other weights is refused; perform_MI_computation(engines=[...]) returns the single-engine frame and files."""
    Ls, N, B = 12_000, 1_000, 3_000
    syn = synth_alignment(Ls, N, seed=1988, device="cuda", as_numpy=False)
    POS, g, paint = syn["POS"], float(syn["g"]), syn["paint"]
    blocks = MIH.make_blocks(Ls, B)
    approx = MIH.lr_links_approx(POS, g, 20000.0)
    engs = [Engine(0) for _ in range(3)]
    try:
        for e in engs:
            e.set_alignment(syn["states"])
        cnt = engs[0].state_counts()
        uqe = (cnt > 0).T.astype(np.float64)
        r = uqe.sum(axis=1)
        thresh = int(Ls * 0.1)
        hdw = engs[0].hamming_weights(thresh)
        for n in (1, 2, 3):
            assert np.array_equal(Engine.hamming_weights_multi(engs[:n], thresh), hdw), n
        for e in engs:
            e.set_weights(hdw)
            e.set_snp_meta(r, uqe, POS, paint, g)

        def tables(e):
            return e.links(0), e.links(1), e.block_stats()

        def same(x, y, what):
            for w in (0, 1):
                for u, v in zip(x[w], y[w]):
                    assert np.array_equal(u, v), (what, w)
            for k in ("n_lr_total", "n_lr_kept", "n_sr"):
                assert np.array_equal(x[2][k], y[2][k]), (what, k)
            assert np.array_equal(x[2]["disc_thresh"], y[2]["disc_thresh"], equal_nan=True), what

        kw = dict(sr_dist=20000.0, lr_retain_links=2e5, lr_links_approx=approx)
        engs[0].reset_speculation()
        engs[0].mi_all_pairs(blocks, **kw)
        one = tables(engs[0])
        engs[0].write_links_tsv(1, str(tmp_path / "one.tsv"))
        assert len(one[0][2]) > 100_000 and len(one[1][2]) > 10_000
        for n in (2, 3):
            for e in engs:
                e.reset_speculation()
            info = Engine.mi_all_pairs_multi(engs[:n], blocks, **kw)
            assert sorted(set(info["owner"].tolist())) == list(range(n)) and len(info["per_engine_ms"]) == n
            same(one, tables(engs[0]), f"{n} contexts")
            engs[0].write_links_tsv(1, str(tmp_path / f"multi{n}.tsv"))
            assert (tmp_path / "one.tsv").read_bytes() == (tmp_path / f"multi{n}.tsv").read_bytes()
            # the other contexts keep their own share
            assert engs[1].links_count(0) == int(one[2]["n_sr"][info["owner"] == 1].sum())
        # (default since the band enumerator builds its intervals on the device: short-range rows travel as their MI column, ctx[0] rebuilds the
        # index columns — ldw_sr_pairs_fill; the other form, and the enumerator's host loop)
        for var in ("LDW_MULTI_SR_FULL_ROWS", "LDW_SR_PAIRS_HOST"):
            os.environ[var] = "1"
            try:
                Engine.mi_all_pairs_multi(engs[:2], blocks, **kw)
                same(one, tables(engs[0]), f"2 contexts, {var}")
            finally:
                os.environ.pop(var)
        # the consumers of the tables run on ctx[0] unchanged: short-range quantiles on the assembled table == on the single-context one
        q_multi = engs[0].sr_len_quantiles(3, 20000.0)
        engs[0].mi_all_pairs(blocks, **kw)
        q_one = engs[0].sr_len_quantiles(3, 20000.0)
        for u, v in zip(q_one, q_multi):
            assert np.array_equal(u, v, equal_nan=True)
        # SR-only parameter set (no long-range part): three-column route
        kw_sr = dict(kw, sr_only=True)
        engs[0].mi_all_pairs(blocks, **kw_sr)
        one_sr = tables(engs[0])
        Engine.mi_all_pairs_multi(engs[:2], blocks, **kw_sr)
        same(one_sr, tables(engs[0]), "2 contexts, sr_only")
        # more contexts than blocks: the idle context is dealt nothing and the result does not change; one context == ldw_mi_all_pairs
        two_blocks = blocks[:2]
        engs[0].mi_all_pairs(two_blocks, **kw)
        one2 = tables(engs[0])
        info = Engine.mi_all_pairs_multi(engs, two_blocks, **kw)
        assert sorted(info["owner"].tolist()) == [0, 1]
        same(one2, tables(engs[0]), "3 contexts, 2 blocks")
        Engine.mi_all_pairs_multi(engs[:1], two_blocks, **kw)
        same(one2, tables(engs[0]), "1 context through the multi entry point")
        # a bad block on one context's share fails the call with that context's message; the engines survive
        bad = blocks.copy()
        bad[len(bad) - 1, 3] = Ls + 9
        with pytest.raises(L.LdwError) as ei:
            Engine.mi_all_pairs_multi(engs[:2], bad, **kw)
        assert "context" in str(ei.value) and "outside 1.." in str(ei.value)
        Engine.mi_all_pairs_multi(engs[:2], blocks, **kw)
        same(one, tables(engs[0]), "2 contexts after a failed call")
        # a context that holds other weights is refused before anything runs
        engs[2].set_weights(np.full(N, 0.25))
        with pytest.raises(L.LdwError) as ei:
            Engine.mi_all_pairs_multi(engs, blocks, **kw)
        assert ei.value.code == L.LDW_ERR_STATE and "context 2" in str(ei.value)
        engs[2].set_weights(hdw)
        # unsorted positions: generic pair lists, all three columns travel
        perm = np.random.default_rng(5).permutation(Ls)
        for e in engs[:2]:
            e.set_snp_meta(r, uqe, POS[perm], paint, g)
        engs[0].mi_all_pairs(blocks, **kw)
        one_u = tables(engs[0])
        Engine.mi_all_pairs_multi(engs[:2], blocks, **kw)
        same(one_u, tables(engs[0]), "2 contexts, unsorted POS")
    finally:
        for e in engs:
            e.close()
    # the host mirror end to end on the reference's bundled sample: perform_MI_computation(engines=[...]) == (engine=...)
    sd = SnpDat.from_states(sample["states"], sample["POS"], sample["g"])
    d1, d2 = tmp_path / "e1", tmp_path / "e2"
    d1.mkdir()
    d2.mkdir()
    args = dict(ncores=1, max_blk_sz=1000, lr_retain_links=1e5, verbose=False, quirk_mode=L.QUIRK_INTENDED)
    with Engine(0) as e1:
        red1 = MIH.perform_MI_computation(sd, sample["hdw"], CdsVar(paint=sample["paint"], nclust=3), lr_save_path=str(d1 / "lr_links.tsv"),
                                          sr_save_path=str(d1 / "sr_links.tsv"), plt_folder=str(d1 / "PLOTS"), engine=e1, **args)
    with Engine(0) as ea, Engine(0) as eb:
        red2 = MIH.perform_MI_computation(sd, sample["hdw"], CdsVar(paint=sample["paint"], nclust=3), lr_save_path=str(d2 / "lr_links.tsv"),
                                          sr_save_path=str(d2 / "sr_links.tsv"), plt_folder=str(d2 / "PLOTS"), engines=[ea, eb], **args)
    _frames_equal(red1, red2)
    assert (d1 / "lr_links.tsv").read_bytes() == (d2 / "lr_links.tsv").read_bytes()
    assert (d1 / "sr_links.tsv").read_bytes() == (d2 / "sr_links.tsv").read_bytes()


def test_paths_agree_on_one_context_across_changing_problems():
    """tools/fuzz_paths.py, three short sequences of random problems (shape, weighting, block size, sr_dist, retention, quirk mode, position layout) run one
    after the other on ONE context: default / verify / no-span paths == the plain path bit for bit, cold and warm, zero screen violations.  Seed 23 from its
    third case on is the sequence that found the stale clean-region flags of r01-r05 (a problem with N = 40 after one with N = 257 read the larger one's flags:
    334 violations); the others are fresh draws."""
    import subprocess
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_paths.py")
    for args in (["--cases", "5", "--seed", "23", "--start", "2"], ["--cases", "12", "--seed", "11"], ["--cases", "12", "--seed", "4242"],
                 ["--cases", "10", "--seed", "401", "--mutate", "mix"]):   # (the last: alignments partly rewritten — copies and complements of SNPs, heavy gaps, 3-5 states, exact halves)
        r = subprocess.run([sys.executable, tool] + args, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "DIFFERENT" not in r.stdout, r.stdout[-3000:] + r.stderr[-1500:]
        assert r.stdout.count(": ok") >= 3


def _mi11(n, pa, pb, W):
    """MI of a biallelic x biallelic pair (r = 2 both, RXY = 1) from the joint weight n of the two flagged states and their marginals (R/computePairwiseMI.R:390-398)."""
    den = W + 2.0
    A0, A1, B0, B1 = pa + 1.0, W - pa + 1.0, pb + 1.0, W - pb + 1.0
    x = n + 0.5
    x01, x10, x11 = A0 - x, B0 - x, den - A0 - B0 + x
    with np.errstate(invalid="ignore", divide="ignore"):
        return (x * np.log(x * den / (A0 * B0)) + x01 * np.log(x01 * den / (A0 * B1)) + x10 * np.log(x10 * den / (A1 * B0)) + x11 * np.log(x11 * den / (A1 * B1))) / den


@pytest.mark.parametrize("W,lo", [(6.614192337876547, 0.98 * 0.314453125), (6.614192337876547, 0.33), (3.0, 0.2), (41.5, 0.5), (41.5, 0.05), (100.0, 0.1), (1000.0, 0.05), (1000.0, 0.62),
                                  (4321.0, 0.2), (4321.0, 0.66)])
def test_threshold_table_never_dismisses_a_pair_that_reaches_the_level(engine, W, lo):
    """The threshold table of the biallelic pairs (k_build_tab11, BOUNDS.md 5) against the MI formula on a grid of joint tables: whenever MI >= lo the sum must lie
    outside (Lq, Hq) of its marginals' bin.  The grid holds what the 3 x 3 corner sampling cannot see by itself: tables on the line pa + pb = W with an EMPTY joint cell
    (perfect anti-association — r05: tools/fuzz_paths.py --seed 203 --only 96 found two such pairs dismissed at W = 6.6, the first parameter set here) and on the
    diagonal pa = pb with a full one, next to a dense sweep.  The table must also still DO something: most tables far below the level are dismissed."""
    import ctypes as C
    s = 2.0 ** -12
    tab = np.zeros(64 * 64 * 2, dtype=np.int32)
    cb = C.c_double(0.0)
    L.check(L.lib().ldw_debug_tab11(engine._ctx, W, lo, 0.0, s, s, L.ptr(tab), C.byref(cb)))
    tab = tab.reshape(64, 64, 2)
    cbin = np.float32(cb.value)
    binof = lambda p: np.minimum(63, (np.sqrt(p.astype(np.float32)) * cbin).astype(np.int64))
    g = np.unique(np.concatenate([np.linspace(0.0, W, 241), (np.arange(65) / float(cbin)) ** 2, W - (np.arange(65) / float(cbin)) ** 2, [W / 2, W / 2 * (1 - 1e-9), W / 2 * (1 + 1e-9)]]))
    g = g[(g >= 0) & (g <= W)]
    pa, pb = np.meshgrid(g, g, indexing="ij")
    pa, pb = pa.ravel(), pb.ravel()
    extra = np.random.default_rng(5).uniform(0.0, W, 4000)     # the two lines, densely
    pa = np.concatenate([pa, extra, extra])
    pb = np.concatenate([pb, W - extra, extra])
    nlo, nhi = np.maximum(0.0, pa + pb - W), np.minimum(pa, pb)
    lost = dismissed_low = low = 0
    for f in np.concatenate([[0.0, 1.0], np.linspace(0.0, 1.0, 41)[1:-1], [1e-6, 1 - 1e-6]]):
        n = nlo + f * (nhi - nlo)
        mi = _mi11(n, pa, pb, W)
        nq = np.rint(n / s).astype(np.int64)    # (the int32 sum of a pair: its error is the eta the table was built with)
        t = tab[binof(pb), binof(pa)]
        dismissed = (nq > t[:, 0]) & (nq < t[:, 1])
        bad = dismissed & (mi >= lo)
        if bad.any():
            k = int(np.argmax(bad))
            raise AssertionError(f"dismissed although MI {mi[k]!r} >= {lo}: pa {pa[k]!r} pb {pb[k]!r} n {n[k]!r} bins {int(binof(pa[k:k+1])[0])} {int(binof(pb[k:k+1])[0])} thresholds {t[k] * s}")
        lost += int(bad.sum())
        sel = mi < 0.5 * lo
        low += int(sel.sum())
        dismissed_low += int((dismissed & sel).sum())
    assert lost == 0
    print(f"W {W} lo {lo}: {dismissed_low} of {low} tables below half the level dismissed")
    assert dismissed_low > 0.6 * low, (dismissed_low, low)


def test_anti_associated_pairs_at_a_small_total_weight_are_not_dismissed(engine):
    """The problem that found the hole above (24 000 SNPs x 130 sequences, Hamming weights summing to 6.6, survey alignment, sr_dist 500.5): verify mode counts no lost
    pair and the default path's tables equal the plain path's."""
    import subprocess
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_paths.py")
    r = subprocess.run([sys.executable, tool, "--cases", "100", "--seed", "203", "--only", "96"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DIFFERENT" not in r.stdout and r.stdout.count(": ok") == 1 and "violations 0" in r.stdout, r.stdout[-3000:] + r.stderr[-1500:]


def test_consumers_of_a_reused_context_equal_a_fresh_one():
    """tools/fuzz_sr_model.py: a sequence of random problems on contexts that are RE-USED from case to case — the short-range model + ARACNE, the Tukey analysis of
    the long-range links and the LD map must equal a fresh context's bit for bit, and the model over two re-used contexts (LDW_MI_SR_ROWS_STAY) the one-table model.
    (It found that a context the in-process deal leaves without a block kept the rows of the problem before.)"""
    import subprocess
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_sr_model.py")
    r = subprocess.run([sys.executable, tool, "--cases", "16", "--seed", "5"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DIFFERENT" not in r.stdout and r.stdout.count(": ok") == 16, r.stdout[-3000:] + r.stderr[-1500:]


def test_default_library_refuses_experiment_variants(engine):
    """The measured-slower variants have been removed: asking for one is an error (LDW_ERR_STATE) that says so, not a silent fallback."""
    assert not L.has_experiments()
    for call in (lambda: engine.set_fused(True), lambda: engine.set_engine(L.ENGINE_HIST_STATES), lambda: engine.set_span(True, 8, corners=True),
                 lambda: engine.set_span(True, 8, diag_split=True)):
        with pytest.raises(L.LdwError) as ei:
            call()
        assert ei.value.code == L.LDW_ERR_STATE and "LDW_EXPERIMENTS" in str(ei.value) and "removed" in str(ei.value)
    engine.set_fused(False)
    engine.set_engine(L.ENGINE_MFMA)
    engine.set_span(True, 8)


def test_lr_links_tsv_streams_while_the_pass_runs(engine, tmp_path):
    """lr_links.tsv is appended item by item WHILE the block loop runs (ldw_lr_stream_begin / _end), like the
    reference's per-block write.table(append = T) (R/computePairwiseMI.R:362).  (a) The streamed file == the file written from the finished
    table, byte for byte — with spans (items of several blocks), without, and with a tiny long-range table that has to GROW during the pass
    (the writer is drained before the table's buffers move).  (b) A pass that fails at block k (a block descriptor outside the alignment:
    the helper threads find it while earlier blocks are still running) leaves EXACTLY the rows of blocks 0..k-1 on disk — the items already
    submitted are run to their end first — and the engine survives.  (c) perform_MI_computation streams by default: same files as with
    stream_lr = False."""
    Ls, N, B = 16_000, 1_000, 2_000
    syn = synth_alignment(Ls, N, seed=1988, device="cuda", as_numpy=False)
    POS, g, paint = syn["POS"], float(syn["g"]), syn["paint"]
    engine.set_engine(L.ENGINE_MFMA)
    engine.set_alignment(syn["states"])
    cnt = engine.state_counts()
    uqe = (cnt > 0).T.astype(np.float64)
    r = uqe.sum(axis=1)
    hdw = engine.hamming_weights(int(Ls * 0.1))
    engine.set_weights(hdw)
    engine.set_snp_meta(r, uqe, POS, paint, g)
    blocks = MIH.make_blocks(Ls, B)      # 8 x 8 grid: 36 block pairs, spans of up to 6
    approx = MIH.lr_links_approx(POS, g, 20000.0)
    kw = dict(sr_dist=20000.0, lr_retain_links=3e5, lr_links_approx=approx)
    engine.reset_speculation()
    engine.mi_all_pairs(blocks, **kw)
    kept = engine.block_stats()["n_lr_kept"]
    whole = tmp_path / "whole.tsv"
    n_rows, n_bytes = engine.write_links_tsv(1, str(whole), append=False)
    assert n_rows == int(kept.sum()) > 100_000
    ref = whole.read_bytes()
    for tag, spans in (("spans", True), ("blocks", False)):
        engine.set_span(spans, 8)
        engine.reset_speculation()
        f = tmp_path / f"stream_{tag}.tsv"
        f.write_bytes(b"stale\n")
        engine.lr_stream_begin(str(f), append=False)
        engine.mi_all_pairs(blocks, **kw)
        rows, nbytes, nblk = engine.lr_stream_end()
        assert (rows, nbytes, nblk) == (n_rows, n_bytes, len(blocks)), (tag, rows, nbytes, nblk)
        assert f.read_bytes() == ref, tag
    engine.set_span(True, 8)
    assert engine.lr_stream_end() == (0, 0, 0)      # no stream open: zeros
    # (b) block k is bad: exactly the rows of the k blocks before it
    lines = ref.split(b"\n")
    for k in (5, 17):       # (block 5: inside the first block row; 17: two rows down)
        bad = blocks.copy()
        bad[k, 3] = Ls + 7
        f = tmp_path / f"fail_{k}.tsv"
        engine.reset_speculation()
        engine.lr_stream_begin(str(f), append=False)
        with pytest.raises(L.LdwError) as ei:
            engine.mi_all_pairs(bad, **kw)
        assert "outside 1.." in str(ei.value)
        rows, nbytes, nblk = engine.lr_stream_end()
        want_rows = int(kept[:k].sum())
        assert nblk == k and rows == want_rows, (k, nblk, rows, want_rows)
        assert f.read_bytes() == b"".join(l + b"\n" for l in lines[:want_rows]), k
    # the engine survives, and a fresh context whose long-range table starts empty grows it under the writer
    with Engine(0) as e2:
        e2.set_alignment(syn["states"])
        e2.set_weights(hdw)
        e2.set_snp_meta(r, uqe, POS, paint, g)
        f = tmp_path / "fresh.tsv"
        e2.lr_stream_begin(str(f), append=True)
        e2.mi_all_pairs(blocks, **kw)
        assert e2.lr_stream_end() == (n_rows, n_bytes, len(blocks))
        assert f.read_bytes() == ref
    # (c) the host mirror
    sd = SnpDat.from_states(syn["states"].cpu().numpy(), POS, g)
    outs = {}
    for stream in (True, False):
        d = tmp_path / f"job_{int(stream)}"
        d.mkdir()
        red, aux = MIH.perform_MI_computation(sd, hdw, CdsVar(paint=paint, nclust=3), lr_save_path=str(d / "lr_links.tsv"), sr_save_path=str(d / "sr_links.tsv"),
                                              plt_folder=str(d / "PLOTS"), max_blk_sz=B, lr_retain_links=3e5, engine=engine, verbose=False, return_aux=True,
                                              stream_lr=stream)
        outs[stream] = ((d / "lr_links.tsv").read_bytes(), (d / "sr_links.tsv").read_bytes(), aux["lr_rows_written"])
    assert outs[True] == outs[False] and outs[True][0] == ref and outs[True][2] == n_rows
