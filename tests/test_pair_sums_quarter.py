"""The exact sums of the listed long-range candidates, a quarter-wave per pair (k_pair_sums_q, ldw_pairs.hip), at the edges of its mapping.

Every case runs one small alignment three ways on fresh engines — the default path (the quarter-wave kernel), the default path with
LDW_PAIR_WAVE=1 (the wave-per-pair kernels) and the plain path — each cold (after reset_speculation) and warm, and compares the short-range
table, the long-range table and block_stats with ==.  ldw_pair_kernel_report proves which kernel ran, path_report that blocks took the
approximate path and listed pairs.

Shapes.  Sequence counts at the word edges of a 16-lane row (a lane holds the 32-bit words 32 k + 2 l, 32 k + 2 l + 1 of a bit row): N = 33
(Npad 128: four words, two lanes of sixteen busy), 513, 1 000 (32 words: one step), 2 049 (Npad 2 176: 68 words, the third step holds two
lanes), 5 000 (160 words: all five steps whose segments stay in registers) and 5 121 (164 words: the first step through the table, two lanes
busy).  At 513 and 5 121 a fourth and a fifth way run the quarter-wave kernel under LDW_PAIR_GRID_WGS=1 and =3, a whole grid of one and three
workgroups per path: a block's few thousand pairs then take dozens of turns of the persistent waves, where the default grid takes one or two (as
functions, against integer sums: tests/test_pair_sums_fn_gpu.py).  L = 2 000 SNPs in blocks of 600: diagonal blocks and single
off-diagonal blocks, square and ragged (spans need blocks of 2 048 SNPs and more: tests/test_gpu_parity.py runs them on the default path).
SNPs with one, two and three minor states at high frequency are planted by clonal group (so that they are in LD with each other over any
distance), and lr_retain_links is 0.65 % of the long-range pairs (a pass speculates up to 0.7 %), so pairs of every shape — the four
straight-line lists and the predicated one — are listed.  Weightings: the Hamming weights of the alignment (a few clonal classes); a hand-set
one whose classes of 1, 2 and 3 sequences are adjacent among large classes, so that 32-bit words hold three and more segments (the table
path of a lane's word); and one case with pair lists of 64 entries, which overflow: the blocks are redone on the plain path.
"""
import os

import numpy as np
import pytest
import torch

from ldweaver_amd import _lib as L
from ldweaver_amd import mi as MIH
from ldweaver_amd.engine import Engine
from ldweaver_amd.synth import synth_alignment

pytestmark = pytest.mark.gpu
LS, BLK = 2_000, 600
SR_DIST = 20000.0
LR_FRAC = 0.0065         # of the long-range pairs: just below the 0.7 % up to which a pass speculates at all


def _alignment(N, seed, Ls=LS, device="cuda"):
    """synth_alignment plus planted multi-state SNPs: every 3rd SNP gets a second minor state in the sequences of every 3rd clonal group,
    every 7th SNP a second and a third one (groups 1 and 2 of 4), every 13th a fourth (state 4) as well.  Group membership is the same for
    every planted SNP, so they are in LD with each other at any distance."""
    syn = synth_alignment(Ls, N, seed=seed, device=device, as_numpy=False)
    st = syn["states"]
    rs = np.random.default_rng(seed + 1)
    grp = torch.as_tensor(rs.integers(0, 12, N), device=st.device)
    rows = torch.arange(Ls, device=st.device)
    base = st[:, :1]                                   # column 0 holds every SNP's major allele (synth_alignment)

    def other(k):                                      # a base k steps from the major one
        return ((base + k) % 4).to(torch.uint8)

    def plant(every, groups, k):
        sel_r = (rows % every == 0)[:, None]
        sel_c = torch.isin(grp % 4, torch.as_tensor(groups, device=st.device))[None, :] & (torch.arange(N, device=st.device) > 0)[None, :]
        st[:] = torch.where(sel_r & sel_c, other(k).expand(-1, N), st)

    plant(3, [1], 1)
    plant(7, [1], 1)
    plant(7, [2], 2)
    plant(13, [1], 1)
    plant(13, [2], 2)
    plant(13, [3], 3)
    return syn


def _hand_weights(N):
    """Classes of 1, 2, 3, 1, 2, 3, ... sequences (48 sequences in 24 adjacent classes) below classes of about N / 12: dyadic values, all
    distinct between classes.  The engine orders the positions by weight, so the small classes share 32-bit words."""
    sizes = [1, 2, 3] * 8
    rest = N - sum(sizes)
    big = [rest // 12] * 12
    big[-1] += rest - sum(big)
    sizes += big
    k = (1 << 16) + 4099 * np.arange(len(sizes))
    w = np.repeat(np.ldexp(k.astype(np.float64), -22), sizes)
    return np.random.default_rng(N).permutation(w)


def _run(syn, hdw, env, plain, pair_cap=0, grid=0):
    """A fresh engine: one cold and one warm pass.  Returns per pass (sr table, lr table, block_stats) and the reports' deltas.
    grid: LDW_PAIR_GRID_WGS, the whole grid of a path of the quarter-wave kernel (read per call)."""
    blocks = MIH.make_blocks(LS, BLK)
    approx = MIH.lr_links_approx(syn["POS"], float(syn["g"]), SR_DIST)
    out = []
    old = os.environ.pop("LDW_PAIR_WAVE", None)
    assert "LDW_PAIR_GRID_WGS" not in os.environ
    try:
        if env:
            os.environ["LDW_PAIR_WAVE"] = "1"
        if grid:
            os.environ["LDW_PAIR_GRID_WGS"] = str(grid)
        Engine.set_pair_cap(pair_cap)
        with Engine(0) as eng:
            eng.set_engine(L.ENGINE_MFMA)
            eng.set_alignment(syn["states"])
            cnt = eng.state_counts()
            uqe = (cnt > 0).T.astype(np.float64)
            r = uqe.sum(axis=1)
            if hdw is None:
                hdw = eng.hamming_weights(int(LS * 0.1))
            eng.set_weights(hdw)
            eng.set_snp_meta(r, uqe, syn["POS"], syn["paint"], float(syn["g"]))
            info = eng.apx_info()
            if plain:
                eng.set_mixed(False)
                eng.set_screen(0)
                eng.set_path(1)
            for cold in (True, False):
                if cold:
                    eng.reset_speculation()
                eng.mi_all_pairs(blocks, SR_DIST, LR_FRAC * approx, approx)
                out.append((eng.links(0), eng.links(1), eng.block_stats()))
            rep = dict(path=eng.path_report(), kern=eng.pair_kernel_report(), form=eng.form_report(), over=eng.overflow_report(),
                       span=eng.span_report(), cnt=eng.counters(), info=info, r=r)
    finally:
        Engine.set_pair_cap(0)
        os.environ.pop("LDW_PAIR_WAVE", None)
        os.environ.pop("LDW_PAIR_GRID_WGS", None)
        if old is not None:
            os.environ["LDW_PAIR_WAVE"] = old
    return out, rep


def _same(x, y, what):
    for which in (0, 1):
        for a, b in zip(x[which], y[which]):
            assert np.array_equal(a, b), (what, which)
    for k in ("n_lr_total", "n_lr_kept", "n_sr", "disc_thresh"):
        assert np.array_equal(x[2][k], y[2][k]), (what, k)


def _three_ways(syn, hdw, pair_cap=0, grids=()):
    plain, rp = _run(syn, hdw, env=False, plain=True)
    quarter, rq = _run(syn, hdw, env=False, plain=False, pair_cap=pair_cap)
    wave, rw = _run(syn, hdw, env=True, plain=False, pair_cap=pair_cap)
    print("quarter:", rq["path"], rq["kern"], rq["form"], rq["over"], rq["span"], rq["info"])
    print("wave:   ", rw["path"], rw["kern"], rw["over"])
    # which kernel ran, on which path
    assert rp["path"]["apx_blocks"] == 0 and rp["kern"] == dict(quarter_wave=0, wave=0), rp
    assert rq["kern"]["quarter_wave"] > 0 and rq["kern"]["wave"] == 0, rq
    assert rw["kern"]["wave"] > 0 and rw["kern"]["quarter_wave"] == 0, rw
    for rep in (rq, rw):
        assert rep["path"]["apx_gate"].startswith("ok") and rep["path"]["apx_blocks"] > 0 and rep["path"]["pairs_listed"] > 0, rep
        assert rep["form"]["classwise_lds"] == rep["kern"]["quarter_wave"] + rep["kern"]["wave"], rep
        assert rep["form"]["bits_lds64"] == 0 and rep["form"]["classwise_global"] == 0, rep
        assert rep["cnt"]["screen_violations"] == 0, rep
    # SNPs of one, two and three minor states are there (state counts 2, 3, 4 and more)
    r = rp["r"]
    assert (r == 2).sum() > 100 and (r == 3).sum() > 100 and (r >= 4).sum() > 50, np.bincount(r.astype(int))
    assert len(plain[0][1][2]) > 5_000 and len(plain[0][0][2]) > 10_000
    for k, tag in enumerate(("cold", "warm")):
        _same(plain[k], quarter[k], ("quarter-wave", tag))
        _same(plain[k], wave[k], ("wave per pair", tag))
    # a fourth and a fifth way: the quarter-wave kernel with a whole grid of `grid` workgroups per path, 16 pairs per workgroup and turn.  Five paths
    # share a block's pairs, so 10 x 16 x grid pairs per block put 32 x grid and more into some path of some block: every wave of it turns twice and more
    for grid in grids:
        forced, rf = _run(syn, hdw, env=False, plain=False, pair_cap=pair_cap, grid=grid)
        per_block = rf["path"]["pairs_listed"] / rf["path"]["apx_blocks"]
        print(f"grid {grid}:", rf["path"], rf["kern"], f"{per_block:.0f} pairs per block = {per_block / (16 * grid):.1f} turns of the grid")
        assert rf["kern"]["quarter_wave"] > 0 and rf["kern"]["wave"] == 0, rf
        assert rf["form"]["classwise_lds"] == rf["kern"]["quarter_wave"] and rf["form"]["bits_lds64"] == 0 and rf["form"]["classwise_global"] == 0, rf
        assert rf["path"]["apx_gate"].startswith("ok") and rf["path"]["apx_blocks"] > 0 and rf["cnt"]["screen_violations"] == 0, rf
        assert per_block >= 10 * 16 * grid, (grid, rf["path"])
        # (a wrong sum can hide behind the fall-back: a block whose candidates miss the guessed bucket is redone on the plain path and the tables
        # come out right.  The grid changes no value, so it changes no block's fate either)
        for k in ("spec_misses", "plain_blocks", "pairs_listed", "units_listed"):
            assert rf["path"][k] == rq["path"][k], (grid, k, rf["path"], rq["path"])
        for k, tag in enumerate(("cold", "warm")):
            _same(plain[k], forced[k], (f"quarter-wave, grid of {grid}", tag))
    return rq, rw


@pytest.mark.parametrize("N", [33, 513, 1000, 2049, 5000, 5121])
def test_quarter_wave_sums_at_the_word_edges_of_a_row(N):
    """Hamming weights (a few clonal classes) at sequence counts around the word edges of a 16-lane row; at 513 and 5 121 (164 words: the first
    step past the registers, two lanes busy) also under whole grids of one and three workgroups, where the persistent waves turn several times."""
    syn = _alignment(N, 100 + N)
    rq, rw = _three_ways(syn, None, grids=(1, 3) if N in (513, 5121) else ())
    assert rq["over"]["pair_list"] == 0 and rw["over"]["pair_list"] == 0, (rq, rw)


@pytest.mark.parametrize("N", [1000, 5000])
def test_quarter_wave_sums_with_three_and_more_segments_in_a_word(N):
    """Hand-set weights with adjacent classes of 1, 2 and 3 sequences: words of three and more segments take the table in LDS."""
    syn = _alignment(N, 200 + N)
    hdw = _hand_weights(N)
    rq, rw = _three_ways(syn, hdw)
    assert rq["info"]["classes"] == 36 and rq["info"]["segments"] > rq["info"]["classes"], rq["info"]
    assert rq["over"]["pair_list"] == 0, rq


def test_quarter_wave_sums_when_a_pair_list_overflows():
    """Pair lists of 64 entries overflow: the kernel works on the clamped lists, the blocks are redone on the plain path, the tables stay equal."""
    syn = _alignment(513, 300)
    rq, rw = _three_ways(syn, None, pair_cap=64)
    # (a block whose list overflowed is recorded as a speculation miss and run again on the plain path; uncapped, the cases above have 0 to 3)
    for rep in (rq, rw):
        assert rep["path"]["spec_misses"] >= 10 and rep["path"]["plain_blocks"] >= 10, rep
