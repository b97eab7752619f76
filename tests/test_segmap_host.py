"""CPU: the segment map's statement (tests/segmap_ref.py) against plain double loops, the two-word split of csrc/ldw_segmap.h compiled for the host against
numpy's rint and the per-SNP summary's rule, the host rules of ldweaver_amd/genemap.py on hand-made integers (sums past 2^63 included), the segment
builders, the exports and ABI names, and the planted example of the gene map through the C oracle alone.  No GPU call."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import c_oracle
import ldw_oracle as orc
import ldweaver_amd
import segmap_ref as G
import snpsum_ref as R
from ldweaver_amd import _lib as L
from ldweaver_amd import background as B
from ldweaver_amd import genemap as GM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_PAIR = (1 << 64) - 1


def bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def key_of(v):
    u = bits(v)
    return (~u) & (2 ** 64 - 1) if u >> 63 else u | (1 << 63)


def loop_map(mi, pos_f, pos_t, g, diag, seg_f, seg_t, S, sr, mask, w_f, w_t, thr, id_f, id_t):
    """Both entries pair by pair, with Python's own integers and round() (half to even) on an exact scaling.  Returns the map with exact sums and, from its
    own maxima, the best pairs."""
    nf, nt = mi.shape
    n = np.zeros((S, S), np.int64)
    nge = np.zeros((S, S), np.int64)
    tot = [[0] * S for _ in range(S)]
    mx = [[None] * S for _ in range(S)]
    members = {}
    npairs = refused = 0
    for a in range(nf):
        for b in range(nt):
            if (a <= b) if diag else (a == b):
                continue
            if seg_f[a] < 0 or seg_t[b] < 0:
                continue
            d = (float(pos_t[b]) - float(pos_f[a])) % g
            cls = 1 if 0.5 * g - abs(d - 0.5 * g) <= sr else 2
            if not cls & mask:
                continue
            v = float(mi[a, b])
            if w_f is not None:
                p = float(w_f[a]) * float(w_t[b])
                v = v - p
            r, c = min(seg_f[a], seg_t[b]), max(seg_f[a], seg_t[b])
            npairs += 1
            n[r, c] += 1
            nge[r, c] += v >= thr
            if abs(v) < 4.0:
                tot[r][c] += round(v * 2.0 ** 40)
            else:
                refused += 1
            if v == v:
                old = mx[r][c]
                mx[r][c] = v if old is None or key_of(v) > key_of(old) else old
            members.setdefault((r, c), []).append((v, (min(id_f[a], id_t[b]) << 32) | max(id_f[a], id_t[b])))
    best = np.full((S, S), NO_PAIR, dtype=np.uint64)
    for (r, c), lst in members.items():
        if mx[r][c] is not None:
            best[r, c] = min(p for v, p in lst if v == v and bits(v) == bits(mx[r][c]))
    mxa = np.array([[np.nan if m is None else m for m in row] for row in mx], dtype=np.float64)
    return dict(n=n, nge=nge, tot=np.array(tot, dtype=object), max=mxa, npairs=npairs, refused=refused, best=best)


@pytest.mark.parametrize("nf,nt,diag", [(1, 1, False), (1, 3, False), (3, 1, False), (7, 5, False), (6, 6, True), (1, 1, True), (9, 9, False), (11, 11, True)])
def test_the_numpy_statement_equals_a_double_loop(nf, nt, diag):
    rng = np.random.default_rng(nf * 100 + nt + 7)
    g, S = 1000.0, 4
    pos_f = rng.integers(1, 1001, nf)
    pos_t = pos_f if diag else rng.integers(1, 1001, nt)
    seg_f = rng.integers(-1, S, nf)
    seg_t = seg_f if diag else rng.integers(-1, S, nt)
    id_f = rng.permutation(50)[:nf] + 60                                        # from-ids above to-ids
    id_t = id_f if diag else rng.permutation(50)[:nt]
    mi = np.where(rng.random((nf, nt)) < 0.2, -rng.random((nf, nt)), np.exp(rng.uniform(-16, 1, (nf, nt))))
    mi.flat[::5] = rng.choice([0.0, -0.0, 1.5 * 2.0 ** -40, 2.5 * 2.0 ** -40, -0.5 * 2.0 ** -40, 4.0, np.inf, np.nan, 0.25], len(mi.flat[::5]))
    w_f = rng.uniform(-0.5, 0.5, nf)
    w_t = w_f if diag else rng.uniform(-0.5, 0.5, nt)
    for sr in (0.0, 120.0, np.inf):
        for mask in (1, 2, 3):
            for wf, wt in ((None, None), (w_f, w_t)):
                ref = loop_map(mi, pos_f, pos_t, g, diag, seg_f, seg_t, S, sr, mask, wf, wt, 0.25, id_f, id_t)
                got = G.segment_map(mi, pos_f, pos_t, g, diag, seg_f, seg_t, S, sr, mask, wf, wt, 0.25)
                assert np.array_equal(got["n"], ref["n"]) and np.array_equal(got["nge"], ref["nge"]) and got["npairs"] == ref["npairs"] == got["n"].sum()
                assert (G.exact(got) == ref["tot"]).all() and got["refused"] == ref["refused"]
                assert (got["sum_lo"] >= 0).all() and R.same_bits(got["max"], ref["max"])
                assert not np.tril(got["n"], -1).any() and np.isnan(got["max"][np.tril_indices(S, -1)]).all()      # only row <= column is written
                best = G.segment_best(mi, pos_f, pos_t, g, diag, seg_f, seg_t, S, sr, mask, id_f, id_t, got["max"], wf, wt)
                assert np.array_equal(best, ref["best"])
    if not diag:                                                                # a pair counts once, whichever side is the from side: the block transposed
        a = G.segment_map(mi, pos_f, pos_t, g, False, seg_f, seg_t, S, 120.0, 2, w_f, w_t, 0.25)
        x = G.segment_map(mi.T, pos_t, pos_f, g, False, seg_t, seg_f, S, 120.0, 2, w_t, w_f, 0.25)
        assert G.same_map(a, x)


def test_cells_are_min_max_and_minus_one_takes_no_part():
    mi = np.arange(1.0, 13.0).reshape(3, 4) / 16
    pos_f, pos_t = np.array([10, 20, 30]), np.array([40, 50, 60, 70])
    seg_f, seg_t = np.array([3, -1, 0]), np.array([1, 3, -1, 0])               # from-segment above the to-segment, below it, and equal
    m = G.segment_map(np.where(np.eye(3, 4, dtype=bool), 0.0, mi), pos_f, pos_t, 1000.0, False, seg_f, seg_t, 4, 5.0, 3)
    # pairs (a, b), a != b, both segments >= 0: (0,1) 3-3, (0,3) 3-0, (2,0) 0-1, (2,1) 0-3, (2,3) 0-0
    expect = np.zeros((4, 4), np.int64)
    expect[3, 3], expect[0, 3], expect[0, 1], expect[0, 0] = 1, 2, 1, 1
    assert np.array_equal(m["n"], expect) and m["npairs"] == 5
    assert m["max"][0, 3] == mi[2, 1] and m["max"][0, 1] == mi[2, 0] and np.isnan(m["max"][1, 0])
    assert m["sum_hi"][0, 3] * 2 ** 24 + m["sum_lo"][0, 3] == int((mi[0, 3] + mi[2, 1]) * 2 ** 40)


def q_values():
    rng = np.random.default_rng(5)
    k = np.arange(0, 40, dtype=np.float64)
    halves = (k + 0.5) * 2.0 ** -40                                             # the half-way cases, even and odd k
    low = np.array([2.0 ** -16 - 2.0 ** -40, 2.0 ** -16, 1 + 2.0 ** -16 - 2.0 ** -40, 3.0 + (2 ** 24 - 1) * 2.0 ** -40])      # all 24 low bits set; a carry into hi
    edge = np.array([0.0, 5e-324, 2.0 ** -41, np.nextafter(2.0 ** -41, 1), np.nextafter(4.0, 0), 4.0, np.nextafter(4.0, 8), 2.0 ** 22, np.inf, np.nan, 1e300])
    v = np.concatenate([halves, low, edge, np.exp(rng.uniform(-40, 1.3, 2000)), rng.uniform(0, 2.0 ** -38, 500)])
    return np.concatenate([v, -v])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_two_word_split_of_the_header_on_the_host(tmp_path):
    exe = str(tmp_path / "segmap_q_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "host", "segmap_q_check.cpp")], check=True, timeout=300)
    v = q_values()
    text = "".join(f"{bits(float(x)):016x}\n" for x in v)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.array([[int(t) for t in line.split()] for line in out.stdout.splitlines()], dtype=np.int64)
    assert got.shape == (len(v), 5)
    q, lo, hi, refused, q21 = got.T
    rlo, rhi, rref = G.q_split(v)
    assert np.array_equal(lo, rlo) and np.array_equal(hi, rhi) and np.array_equal(refused.astype(bool), rref)
    assert np.array_equal(hi * 2 ** 24 + lo, q) and (lo >= 0).all() and (lo < 2 ** 24).all() and np.abs(q).max() == 2 ** 42      # (the double below 4 rounds to 2^42 itself)
    with np.errstate(invalid="ignore"):
        inside = np.abs(v) < 4.0
    assert np.array_equal(q[inside], q21[inside]) and np.array_equal(q21[inside], R.q_fixed(v[inside])[0])      # snpsum_q's product and rounding
    assert not q[~inside].any() and rref.sum() == (~inside).sum() == 2 * 6      # 4, its upper neighbour, 2^22, inf, NaN and 1e300, both signs
    assert (lo == 2 ** 24 - 1).sum() >= 3 and (q < 0).sum() > 1000             # the mask and the arithmetic shift are exercised
    lo1, hi1, _ = G.q_split(np.array([-2.0 ** -40, -(2.0 ** -16), -(2.0 ** -16) - 2.0 ** -40]))
    assert lo1.tolist() == [2 ** 24 - 1, 0, 2 ** 24 - 1] and hi1.tolist() == [-1, -1, -2]


def hand_made(pair=True):
    S = 3
    one = 1 << 40
    n = np.array([[2, 4, 0], [0, 1, 8], [0, 0, 4]], dtype=np.int64)
    nge = np.array([[1, 4, 0], [0, 0, 4], [0, 0, 1]], dtype=np.int64)
    tot = [[one, 2 * one, 0], [0, -one // 2, 2 * one], [0, 0, 3 * one]]
    lo = np.array([[t & (2 ** 24 - 1) for t in row] for row in tot], dtype=np.int64)
    hi = np.array([[t >> 24 for t in row] for row in tot], dtype=np.int64)
    mx = np.array([[0.75, 1.0, np.nan], [np.nan, -0.5, 1.0], [np.nan, np.nan, 2.0]])
    pr = np.full((S, S), NO_PAIR, dtype=np.uint64)
    pr[0, 1], pr[1, 2], pr[0, 0] = (0 << 32) | 3, (2 << 32) | 4, (0 << 32) | 1
    POS = np.array([10, 20, 30, 40, 50], dtype=np.int32)
    return GM.GeneMap(n, nge, lo, hi, mx, pr if pair else None, int(n.sum()), np.array([0, 0, 1, 1, 2], np.int32), POS, 0.5, "lr", 15.0)


def test_genemap_methods_on_hand_made_integers():
    gm = hand_made()
    assert gm.S == 3
    assert np.array_equal(gm.mean(), [[0.5, 0.5, np.nan], [np.nan, -0.5, 0.25], [np.nan, np.nan, 0.75]], equal_nan=True)
    assert np.array_equal(gm.frac(), [[0.5, 1.0, np.nan], [np.nan, 0.0, 0.5], [np.nan, np.nan, 0.25]], equal_nan=True)
    es = gm.exact_sum()
    assert es.dtype == object and es[1, 1] == -(1 << 39) and es[2, 2] == 3 << 40 and isinstance(es[0, 1], int)
    sym = gm.symmetric("n")
    assert np.array_equal(sym, sym.T) and sym[1, 0] == 4 and sym[2, 1] == 8 and sym[1, 1] == 1
    assert gm.symmetric("max")[2, 1] == 1.0 and np.isnan(gm.symmetric("mean")[2, 0]) and gm.symmetric("exact_sum")[1, 0] == 2 << 40
    with pytest.raises(ValueError):
        gm.symmetric("pairs")
    fr = gm.frame()
    assert list(fr.columns) == ["seg1", "seg2", "n", "nge", "frac", "mean", "max", "pos1", "pos2"]
    # off-diagonal cells with a pair: (0, 1) and (1, 2), tied at nge 4: the smaller (seg1, seg2) first
    assert fr[["seg1", "seg2"]].values.tolist() == [[0, 1], [1, 2]] and fr["nge"].tolist() == [4, 4]
    assert fr["pos1"].tolist() == [10.0, 30.0] and fr["pos2"].tolist() == [40.0, 50.0]
    by_mean = gm.frame(by="mean", include_diagonal=True)
    assert by_mean[["seg1", "seg2"]].values.tolist() == [[2, 2], [0, 0], [0, 1], [1, 2], [1, 1]]      # 0.75, 0.5, 0.5 (tie: (0,0) before (0,1)), 0.25, -0.5
    assert np.isnan(by_mean["pos1"][0]) and by_mean["pos1"][1] == 10.0 and by_mean["pos2"][1] == 20.0      # (2, 2) names no pair
    by_max = gm.frame(by="max", include_diagonal=True, top=2)
    assert by_max[["seg1", "seg2"]].values.tolist() == [[2, 2], [0, 1]]         # 2.0, then 1.0 twice: (0, 1) before (1, 2)
    assert gm.frame(min_pairs=5)[["seg1", "seg2"]].values.tolist() == [[1, 2]] and len(gm.frame(top=0)) == 0
    with pytest.raises(ValueError):
        gm.frame(by="frac")
    nb = hand_made(pair=False).frame()
    assert np.isnan(nb["pos1"]).all() and np.isnan(nb["pos2"]).all() and nb["n"].tolist() == [4, 8]
    from ldweaver_amd import plots
    h = plots.gene_map_matrix(gm, "mean")
    assert h.shape == (3, 3) and np.array_equal(h, h.T) and h.max() == 1.0 and h[2, 2] == 1.0 and h[1, 1] == 0.0 and h[0, 2] == 0.0 and h[0, 1] == 0.5 / 0.75
    assert np.array_equal(plots.gene_map_matrix(gm, "frac")[0], [0.5, 1.0, 0.0])
    with pytest.raises(ValueError):
        plots.gene_map_matrix(gm, "nge")


def test_sums_past_2_63_stay_exact():
    """A cell of 2^38 pairs of value 3.5: the exact sum 2^38 * 3.5 * 2^40 is near 2^80; each word stays inside int64 and the host never leaves integers."""
    npair = 1 << 38
    q = 7 << 39                                                                 # 3.5 in fixed point
    lo_w, hi_w = q & (2 ** 24 - 1), q >> 24
    q2 = (1 << 40) + 0xABCDEF                                                    # a value with low bits: 1 + 0xABCDEF 2^-40
    n = np.array([[npair, npair], [0, 3]], dtype=np.int64)
    lo = np.array([[npair * lo_w, npair * (q2 & (2 ** 24 - 1))], [0, 5]], dtype=np.int64)
    hi = np.array([[npair * hi_w, npair * (q2 >> 24)], [0, 0]], dtype=np.int64)
    assert int(hi[0, 0]) * 2 ** 24 > 2 ** 63 and int(lo[0, 1]) > 2 ** 53        # neither int64 nor a double holds the sum
    gm = GM.GeneMap(n, np.zeros((2, 2), np.int64), lo, hi, np.array([[3.5, 2.0], [np.nan, 0.5]]), None, int(n.sum()), np.zeros(2, np.int32), np.array([1, 2]), np.inf,
                    "all", 0.0)
    es = gm.exact_sum()
    assert es[0, 0] == npair * q and es[0, 1] == npair * q2 and es[1, 1] == 5
    m = gm.mean()
    assert m[0, 0] == 3.5 and m[0, 1] == 1.0 + 0xABCDEF * 2.0 ** -40 and m[1, 1] == 5 / 3 / 2.0 ** 40 and np.isnan(m[1, 0])
    fr = gm.frame(by="mean", include_diagonal=True)
    assert fr["mean"].tolist() == [3.5, 1.0 + 0xABCDEF * 2.0 ** -40, 5 / 3 / 2.0 ** 40] and fr["n"].tolist() == [npair, npair, 3]


def test_segments_from_features():
    pos = np.array([5, 10, 11, 20, 21, 30, 50, 7], dtype=np.int32)
    #            feature 0: 10..20, 1: 15..30 (overlaps 0), 2: 1..5, 3: 10..10 (inside 0), 4: 60..70 (holds none)
    seg = GM.segments_from_features(pos, [10, 15, 1, 10, 60], [20, 30, 5, 10, 70])
    assert seg.dtype == np.int32 and seg.tolist() == [2, 0, 0, 0, 1, 1, -1, -1]       # both ends inclusive; the smallest index wins an overlap; 50 and 7 in none
    assert GM.segments_from_features(pos, [], []).tolist() == [-1] * 8
    assert GM.segments_from_features(np.array([3, 3, 1]), [3], [3]).tolist() == [0, 0, -1]      # repeated positions
    rng = np.random.default_rng(2)
    p = rng.integers(1, 500, 300)
    st = rng.integers(1, 500, 40)
    en = st + rng.integers(0, 60, 40)
    brute = np.array([next((j for j in range(40) if st[j] <= x <= en[j]), -1) for x in p])
    assert np.array_equal(GM.segments_from_features(p, st, en), brute)
    with pytest.raises(ValueError):
        GM.segments_from_features(pos, [1, 2], [3])


def test_segments_from_annotation_and_equal():
    from types import SimpleNamespace
    from ldweaver_amd.cds import Annotation
    ann = Annotation.from_arrays([10, 15, 40], [20, 30, 45], "A" * 60)
    snp = SimpleNamespace(POS=np.array([9, 10, 25, 33, 45], dtype=np.int32))
    seg, table = GM.segments_from_annotation(snp, gff=ann)
    assert seg.tolist() == [-1, 0, 1, -1, 2] and list(table.columns) == ["start", "end", "strand"] and table["start"].tolist() == [10, 15, 40]
    assert table["strand"].tolist() == ["+"] * 3
    assert GM.segments_from_annotation(snp, gff=ann, feature="gene")[0].tolist() == [-1] * 5
    with pytest.raises(ValueError):
        GM.segments_from_annotation(snp)
    g = 1000
    assert GM.segments_equal([1, g, 250, 251, 500, 501], g, 4).tolist() == [0, 3, 0, 1, 1, 2]      # pos = 1 -> 0; pos = g -> n - 1; stretches (0, 250], (250, 500], ...
    assert GM.segments_equal([1, 7, 8], 7, 7).tolist() == [0, 6, 6] and GM.segments_equal([1, 5], 5, 1).tolist() == [0, 0]      # a position past g is clamped
    assert GM.segments_equal(np.array([2 ** 31 - 1]), 2 ** 31 - 1, 8192).tolist() == [8191]                                      # no 32-bit overflow
    with pytest.raises(ValueError):
        GM.segments_equal([1], 10, 0)


def test_exports():
    for name in ("gene_map", "GeneMap", "segments_from_features", "segments_from_annotation", "segments_equal"):
        assert name in ldweaver_amd.__all__ and getattr(ldweaver_amd, name) is getattr(GM, name)
    from ldweaver_amd import plots
    from ldweaver_amd.engine import Engine
    assert callable(plots.gene_map_plot)
    for name in ("mi_segment_map", "mi_segment_best", "segment_map_report", "debug_segment_map", "debug_segment_best"):
        assert callable(getattr(Engine, name))
    api, debug = {"ldw_mi_segment_map", "ldw_mi_segment_best"}, {"ldw_debug_segment_map", "ldw_debug_segment_best", "ldw_segment_map_report"}
    for name in api | debug:
        assert name in L.declared_symbols() and hasattr(L.lib(), name)
    assert api <= set(L.declared_symbols("ldweaver_amd.h")) and debug <= set(L.declared_symbols("ldweaver_amd_debug.h"))
    assert not api & set(L.declared_symbols("ldweaver_amd_debug.h")) and not debug & set(L.declared_symbols("ldweaver_amd.h"))
    with open(os.path.join(ROOT, "ldweaver_amd", "csrc", "ldw_segmap.hip")) as f:      # LDW_ERR_SIZE is not reachable at test sizes: read, not run
        src = f.read()
    assert "total < (int64_t(1) << 39), LDW_ERR_SIZE" in src


def planted_on_the_oracle():
    """The planted example's values from the C oracle, its background from the per-SNP statement, and the two maps from the segment statement."""
    st, pos, g, sr, seg, marker_segs, cell, pairs = G.planted_genes()
    uqe, r = orc.uqe_r(st)
    idx = np.arange(len(st))
    M = c_oracle.mi_block(st, np.ones(st.shape[1]), r, uqe, idx, idx)
    rows, cols, npairs, _ = R.snp_summary(M, pos, pos, g, True, sr, (np.inf, np.inf))
    tot = R.empty_total(len(st))
    R.fold(tot, rows, idx)
    R.fold(tot, cols, idx)
    bg = B.SnpBackground(tot["n"], tot["sumq"], tot["max"], tot["nge"], npairs, pos, g, sr, (np.inf, np.inf))
    w = B.apc_weights(bg, "lr")
    raw = G.segment_map(M, pos, pos, g, True, seg, seg, 12, sr, 2, thr=G_THR)
    apc = G.segment_map(M, pos, pos, g, True, seg, seg, 12, sr, 2, w, w, thr=G_THR)
    best = G.segment_best(M, pos, pos, g, True, seg, seg, 12, sr, 2, idx, idx, apc["max"], w, w)
    return raw, apc, best, (seg, marker_segs, cell, pairs, pos)


G_THR = 0.2                                                                     # between the planted pairs' values and the corrected marker pairs'


def as_genemap(m, pair, seg, pos, sr):
    return GM.GeneMap(m["n"], m["nge"], m["sum_lo"], m["sum_hi"], m["max"], pair, m["npairs"], seg, pos, G_THR, "lr", sr)


def test_the_planted_example_through_the_c_oracle():
    """Four marker segments and one planted cell: by raw nge the six marker cells rank first, every one of their 100 pairs above the threshold; with the
    average product correction the planted cell ranks first, no other cell holds a pair above the threshold, and its best pair is a planted pair."""
    raw, apc, best, (seg, marker_segs, cell, pairs, pos) = planted_on_the_oracle()
    assert raw["npairs"] == apc["npairs"] == 120 * 119 // 2 and raw["refused"] == 0
    fr = as_genemap(raw, None, seg, pos, 500.0).frame()
    marker_cells = {(a, b) for a in marker_segs for b in marker_segs if a < b}
    assert {(int(a), int(b)) for a, b in fr[["seg1", "seg2"]].values[:6]} == marker_cells and (fr["nge"][:6] == 100).all()
    assert tuple(fr[["seg1", "seg2"]].values[6]) == cell and fr["nge"][6] == 5
    fa = as_genemap(apc, best, seg, pos, 500.0).frame()
    print("corrected: planted nge", fa["nge"][0], "max", fa["max"][0], "next nge", fa["nge"][1], "largest marker max", max(apc["max"][c] for c in marker_cells))
    assert tuple(fa[["seg1", "seg2"]].values[0]) == cell and fa["nge"][0] == 5 and fa["nge"][1] == 0
    assert max(apc["max"][c] for c in marker_cells) < 0.5 * G_THR
    p = int(best[cell])
    assert (p >> 32, p & 0xFFFFFFFF) in pairs and (fa["pos1"][0], fa["pos2"][0]) == (float(pos[p >> 32]), float(pos[p & 0xFFFFFFFF]))
    by_max = as_genemap(apc, best, seg, pos, 500.0).frame(by="max")
    assert tuple(by_max[["seg1", "seg2"]].values[0]) == cell
