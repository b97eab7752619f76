"""CPU: the per-SNP MI summary's statement (tests/snpsum_ref.py) against a double loop, the host rules of ldweaver_amd/background.py on hand-made integers,
the exports and ABI names, the fixed-point rule of csrc/ldw_snpsum.h compiled for the host against numpy's rint, and the planted example of the average
product correction through the C oracle alone.  No GPU call."""
import os
import shutil
import struct
import subprocess
import warnings

import numpy as np
import pandas as pd
import pytest

import c_oracle
import decay_ref as D
import ldw_oracle as orc
import ldweaver_amd
import snpsum_ref as R
from ldweaver_amd import _lib as L
from ldweaver_amd import background as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def key_of(v):
    u = bits(v)
    return (~u) & (2 ** 64 - 1) if u >> 63 else u | (1 << 63)


def loop_summary(mi, pos_f, pos_t, g, diag, sr, thr):
    """The statement pair by pair, with Python's own integers and round() (half to even) on an exact scaling."""
    nf, nt = mi.shape
    new = lambda k: dict(n=np.zeros((2, k), np.int64), sumq=[[0] * k, [0] * k], max=[[None] * k, [None] * k], nge=np.zeros((2, k), np.int64))
    rows, cols, npairs, refused = new(nf), new(nt), [0, 0], 0
    for a in range(nf):
        for b in range(nt):
            if (a <= b) if diag else (a == b):
                continue
            d = (float(pos_t[b]) - float(pos_f[a])) % g
            c = 0 if 0.5 * g - abs(d - 0.5 * g) <= sr else 1
            v = float(mi[a, b])
            if abs(v) < 2.0 ** 22:
                q = round(v * 2.0 ** 40)
            else:
                q, refused = 0, refused + 1
            npairs[c] += 1
            for side, i in ((rows, a), (cols, b)):
                side["n"][c, i] += 1
                side["sumq"][c][i] += q
                side["nge"][c, i] += v >= thr[c]
                old = side["max"][c][i]
                side["max"][c][i] = v if old is None or key_of(v) > key_of(old) else old
    for side in (rows, cols):
        side["sumq"] = np.array(side["sumq"], dtype=np.int64)
        side["max"] = np.array([[np.nan if m is None else m for m in r] for r in side["max"]], dtype=np.float64)
    return rows, cols, np.array(npairs), refused


@pytest.mark.parametrize("nf,nt,diag", [(1, 1, False), (1, 2, False), (2, 1, False), (7, 5, False), (6, 6, True), (1, 1, True), (9, 9, False)])
def test_the_numpy_statement_equals_a_double_loop(nf, nt, diag):
    rng = np.random.default_rng(nf * 100 + nt)
    g = 1000.0
    pos_f = rng.integers(1, 1001, nf)
    pos_t = pos_f if diag else rng.integers(1, 1001, nt)
    mi = np.where(rng.random((nf, nt)) < 0.2, -rng.random((nf, nt)), np.exp(rng.uniform(-16, 1, (nf, nt))))
    mi.flat[::5] = rng.choice([0.0, -0.0, 1.5 * 2.0 ** -40, 2.5 * 2.0 ** -40, -0.5 * 2.0 ** -40, 2.0 ** 22, np.inf, 0.25], len(mi.flat[::5]))
    thr = (0.25, 0.01)
    for sr in (0.0, 120.0, 500.0, np.inf):
        rows, cols, npairs, refused = R.snp_summary(mi, pos_f, pos_t, g, diag, sr, thr)
        rows2, cols2, npairs2, refused2 = loop_summary(mi, pos_f, pos_t, g, diag, sr, thr)
        assert R.same_side(rows, rows2) and R.same_side(cols, cols2) and np.array_equal(npairs, npairs2) and refused == refused2
        assert npairs.sum() == (nf * (nf - 1) // 2 if diag else nf * nt - min(nf, nt))
        assert np.array_equal(rows["n"].sum(axis=1), npairs) and np.array_equal(cols["n"].sum(axis=1), npairs)
    tot = R.empty_total(nf + nt)                                               # folding the two sides: every pair at both of its SNPs
    R.fold(tot, rows, np.arange(nf))
    R.fold(tot, cols, nf + np.arange(nt))
    assert np.array_equal(tot["n"].sum(axis=1), 2 * npairs) and tot["sumq"].sum() == 2 * rows["sumq"].sum()


def q_values():
    rng = np.random.default_rng(40)
    k = np.concatenate([np.arange(0, 9), [1000, 1001, 2 ** 38, 2 ** 38 + 1, 2 ** 51, 2 ** 51 + 1]]).astype(np.float64)
    halves = (k + 0.5) * 2.0 ** -40
    edge = np.array([2.0 ** 22, D.below(2.0 ** 22), np.nextafter(2.0 ** 22, np.inf), np.inf, np.nan, 0.0, 5e-324, 1e-310, 2.0 ** -41, D.below(2.0 ** -41),
                     np.nextafter(2.0 ** -41, 1.0), 1.6094379124341003, 1e300])
    v = np.concatenate([halves, edge, np.exp(rng.uniform(-40, 15, 2000)), rng.uniform(0, 2.0 ** -38, 500)])
    return np.concatenate([v, -v])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_fixed_point_rule_of_the_header_on_the_host(tmp_path):
    exe = str(tmp_path / "snpsum_q_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "host", "snpsum_q_check.cpp")], check=True, timeout=300)
    v = q_values()
    text = "".join(f"{bits(float(x)):016x}\n" for x in v)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.array([[int(t) for t in line.split()] for line in out.stdout.splitlines()], dtype=np.int64)
    assert got.shape == (len(v), 2)
    q, refused = R.q_fixed(v)
    assert np.array_equal(got[:, 0], q) and np.array_equal(got[:, 1].astype(bool), refused)
    assert refused.sum() == 2 * 5 and np.abs(q).max() < 2 ** 62                # 2^22, its upper neighbour, inf, NaN and 1e300, both signs
    assert R.q_fixed(np.array([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5]) * 2.0 ** -40)[0].tolist() == [0, 2, 2, 4, 0, -2, -2]


def test_exports():
    for name in ("snp_background", "SnpBackground", "link_apc"):
        assert name in ldweaver_amd.__all__ and getattr(ldweaver_amd, name) is getattr(B, name)
    from ldweaver_amd import plots
    from ldweaver_amd.engine import Engine
    assert callable(plots.snp_background_plot)
    for name in ("mi_snp_summary", "snp_summary_report", "debug_snp_summary"):
        assert callable(getattr(Engine, name))
    for name in ("ldw_mi_snp_summary", "ldw_debug_snp_summary", "ldw_snp_summary_report"):
        assert name in L.declared_symbols() and hasattr(L.lib(), name)
    assert "ldw_mi_snp_summary" in L.declared_symbols("ldweaver_amd.h")
    assert {"ldw_debug_snp_summary", "ldw_snp_summary_report"} <= set(L.declared_symbols("ldweaver_amd_debug.h"))


def hand_made():
    one = 1 << 40
    n = np.array([[2, 0, 1, 4], [2, 4, 0, 12]], dtype=np.int64)
    sumq = np.array([[one, 0, one // 2, 2 * one], [3 * one, one, 0, 0]], dtype=np.int64)
    mx = np.array([[0.75, np.nan, 0.5, 1.0], [2.0, 0.5, np.nan, 0.0]])
    nge = np.zeros((2, 4), dtype=np.int64)
    return B.SnpBackground(n, sumq, mx, nge, np.array([5, 11]), np.array([10, 20, 30, 40], dtype=np.int32), 1000.0, 15.0, (np.inf, np.inf))


def test_background_methods_on_hand_made_integers():
    bg = hand_made()
    assert np.array_equal(bg.mean("sr"), [0.5, np.nan, 0.5, 0.5], equal_nan=True)
    assert np.array_equal(bg.mean("lr"), [1.5, 0.25, np.nan, 0.0], equal_nan=True)
    assert np.array_equal(bg.mean("all"), [1.0, 0.25, 0.5, 0.125])            # the class sum: SNP 3 has (2 + 0) / (4 + 12), not the mean of 0.5 and 0
    assert bg.mean("all")[3] != np.mean([bg.mean("sr")[3], bg.mean("lr")[3]])
    assert bg.overall_mean("sr") == 3.5 / 7 and bg.overall_mean("lr") == 4.0 / 18 and bg.overall_mean("all") == 7.5 / 25
    empty = B.SnpBackground(np.zeros((2, 3), np.int64), np.zeros((2, 3), np.int64), np.full((2, 3), np.nan), np.zeros((2, 3), np.int64), np.zeros(2, np.int64),
                            np.arange(3), 10.0, 1.0, (0.0, 0.0))
    assert np.isnan(empty.mean("all")).all() and np.isnan(empty.overall_mean("lr"))
    with pytest.raises(ValueError):
        bg.mean("long")
    h = bg.hubs("lr", 2)
    assert list(h.columns) == ["snp", "pos", "n", "mean"] and h["snp"].tolist() == [0, 1] and h["pos"].tolist() == [10, 20] and h["mean"].tolist() == [1.5, 0.25]
    assert bg.hubs("lr", 10)["snp"].tolist() == [0, 1, 3]                      # SNP 2 has no long-range partner
    fr = bg.frame()
    assert list(fr.columns) == ["pos", "n_sr", "mean_sr", "max_sr", "nge_sr", "n_lr", "mean_lr", "max_lr", "nge_lr"] and len(fr) == 4
    assert fr["n_lr"].tolist() == [2, 4, 0, 12] and np.isnan(fr["max_lr"][2])


def test_link_apc_arithmetic_rows_and_order():
    bg = hand_made()
    links = pd.DataFrame({"pos1": [40, 10, 20, 10], "pos2": [10, 20, 40, 30], "MI": [1.0, 0.5, 0.25, 2.0], "tag": ["a", "b", "c", "d"]})
    before = links.copy()
    out = B.link_apc(links, bg)
    assert links.equals(before)                                                 # the caller's frame is untouched
    assert list(out.columns) == ["pos1", "pos2", "MI", "tag", "bg1", "bg2", "apc", "mi_apc"] and out[["pos1", "pos2", "MI", "tag"]].equals(before)
    overall = 4.0 / 18
    assert np.array_equal(out["bg1"], [0.0, 1.5, 0.25, 1.5]) and np.array_equal(out["bg2"], [1.5, 0.25, 0.0, np.nan], equal_nan=True)
    assert np.array_equal(out["apc"], np.array([0.0, 1.5 * 0.25, 0.0, np.nan]) / overall, equal_nan=True)
    assert np.array_equal(out["mi_apc"], before["MI"] - out["apc"], equal_nan=True)
    allc = B.link_apc(links, bg, which="all")
    assert allc["apc"][1] == 1.0 * 0.25 / (7.5 / 25)
    from types import SimpleNamespace
    same = B.link_apc(links, bg, SimpleNamespace(POS=np.array([10, 20, 30, 40])))
    assert same.equals(out)
    with pytest.raises(ValueError, match="not a SNP position"):
        B.link_apc(pd.DataFrame({"pos1": [10], "pos2": [25], "MI": [1.0]}), bg)
    with pytest.raises(ValueError, match="no MI column"):
        B.link_apc(pd.DataFrame({"pos1": [10], "pos2": [20]}), bg)
    assert len(B.link_apc(links.iloc[:0], bg)) == 0


def test_sums_over_the_snps_do_not_wrap():
    """Every SNP's sumq is below 2^62, their sum over the SNPs is not below 2^63: overall_mean and link_apc take it in Python's integers."""
    big = 1 << 61                                                              # MI 2^21 in fixed point: six of them pass 2^63
    L_ = 6
    n = np.full((2, L_), 4, dtype=np.int64)
    sumq = np.stack([np.full(L_, big, dtype=np.int64), np.array([big, big - 3, big, 5, big, big], dtype=np.int64)])
    assert int(sumq[0].sum()) < 0                                              # int64 wraps here
    assert B.exact_sum(sumq[0]) == 6 * big and B.exact_sum(sumq[1]) == 5 * big + 2 and B.exact_sum(-sumq) == -(11 * big + 2)
    assert B.exact_sum(np.zeros(0, dtype=np.int64)) == 0 and B.exact_sum(np.array([-1, 1 << 62, -(1 << 62)])) == -1
    bg = B.SnpBackground(n, sumq, np.full((2, L_), np.nan), np.zeros((2, L_), np.int64), np.array([12, 12]), 10 * np.arange(1, L_ + 1), 1000.0, 15.0,
                         (np.inf, np.inf))
    assert bg.overall_mean("sr") == 6 * big / 24 / 2.0 ** 40 == 2.0 ** 19
    assert bg.overall_mean("lr") == (5 * big + 2) / 24 / 2.0 ** 40 and bg.overall_mean("all") == (11 * big + 2) / 48 / 2.0 ** 40
    assert bg.overall_mean("lr") > 0 and bg.overall_mean("all") > 0
    assert np.array_equal(bg.mean("sr"), np.full(L_, 2.0 ** 19)) and bg.mean("all")[0] == 2.0 ** 19      # per SNP the two classes still fit
    out = B.link_apc(pd.DataFrame({"pos1": [10, 40], "pos2": [20, 10], "MI": [2.0 ** 20, 1.0]}), bg, which="sr")
    assert np.array_equal(out["apc"], [2.0 ** 19, 2.0 ** 19]) and np.array_equal(out["mi_apc"], [2.0 ** 19, 1.0 - 2.0 ** 19])
    lr = B.link_apc(pd.DataFrame({"pos1": [10], "pos2": [40], "MI": [0.0]}), bg, which="lr")
    assert lr["apc"][0] == bg.mean("lr")[0] * bg.mean("lr")[3] / bg.overall_mean("lr") > 0


def test_link_apc_warns_once_when_the_overall_mean_is_zero():
    bg = hand_made()
    bg.sumq[:] = 0
    links = pd.DataFrame({"pos1": [10, 20], "pos2": [20, 40], "MI": [1.0, 0.5]})
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = B.link_apc(links, bg)
    assert len(w) == 1 and issubclass(w[0].category, RuntimeWarning)
    assert np.isnan(out["apc"]).all() and np.isnan(out["mi_apc"]).all()


def test_the_planted_example_through_the_c_oracle():
    """Forty lineage markers and one planted pair: by raw MI all 780 marker pairs rank above the planted pair; by mi_apc, from the statement applied to the
    C oracle's MI, the planted pair ranks first and no marker pair reaches half of it."""
    st, pos, g, sr, markers, (pa, pb) = R.planted_apc()
    uqe, r = orc.uqe_r(st)
    idx = np.arange(len(st))
    M = c_oracle.mi_block(st, np.ones(st.shape[1]), r, uqe, idx, idx)          # the C oracle; the numpy restatement agrees with it to 1e-12
    assert np.abs(M - orc.mi_block_faithful(st, np.ones(st.shape[1]), r, uqe, idx, idx)).max() < 1e-12
    rows, cols, npairs, refused = R.snp_summary(M, pos, pos, g, True, sr, (np.inf, np.inf))
    assert npairs.tolist() == [0, 120 * 119 // 2] and refused == 0
    tot = R.empty_total(len(st))
    R.fold(tot, rows, idx)
    R.fold(tot, cols, idx)
    bg = B.SnpBackground(tot["n"], tot["sumq"], tot["max"], tot["nge"], npairs, pos, g, sr, (np.inf, np.inf))
    a, b = np.tril_indices(len(st), -1)
    links = B.link_apc(pd.DataFrame({"pos1": pos[a], "pos2": pos[b], "MI": M[a, b]}), bg)
    is_marker = np.isin(a, markers) & np.isin(b, markers)
    planted = np.flatnonzero((a == max(pa, pb)) & (b == min(pa, pb)))
    assert is_marker.sum() == 780 and len(planted) == 1
    p = int(planted[0])
    raw, apc = links["MI"].to_numpy(), links["mi_apc"].to_numpy()
    print("planted raw", raw[p], "marker raw min", raw[is_marker].min(), "planted mi_apc", apc[p], "marker mi_apc max", apc[is_marker].max())
    assert raw[is_marker].min() > raw[p]
    assert int(np.argmax(apc)) == p
    assert apc[is_marker].max() < 0.5 * apc[p]
