"""CPU: create_tanglegram's selection (segments, links, locus lookup) against the naive counterparts of tests/tanglegram_ref.py, its layout's
integer rules and its refusals.  No GPU: nothing is drawn without a folder."""
import warnings

import numpy as np
import pandas as pd
import pytest
from scipy.cluster.hierarchy import fcluster, linkage

import ldweaver_amd
import tanglegram_ref as TR
from ldweaver_amd import network as N
from ldweaver_amd import tanglegram as T
from ldweaver_amd.cds import Annotation
from ldweaver_amd.gbk import GenBankRecord


def record(tags, starts, ends):
    n = len(tags)
    cds = pd.DataFrame({"seqnames": ["chr"] * n, "start": np.asarray(starts, dtype=np.int64), "end": np.asarray(ends, dtype=np.int64), "strand": ["+"] * n,
                        "type": ["CDS"] * n, "locus_tag": list(tags), "gene": [""] * n, "product": [""] * n})
    return GenBankRecord(cds=cds, sequence=np.zeros(0, dtype=np.uint8), seqname="chr", g=0)


def annotation(attrs, starts, ends):
    a = Annotation.from_arrays(starts, ends, "ACGT")
    a.gff["attributes"] = list(attrs)
    return a


def genome(n_genes=30, step=4000):
    """Genes G000, G001, ... of 900 bp every ``step`` bp."""
    tags = [f"G{j:03d}" for j in range(n_genes)]
    starts = [1000 + step * j for j in range(n_genes)]
    return tags, starts, [s + 899 for s in starts]


def make_tophits(n=60, seed=3, n_genes=30, step=4000):
    """About n rows in three stretches of the genome (genes 0..5, 12..17, 24..29), rows in shuffled order, few distinct pairs per stretch."""
    rng = np.random.default_rng(seed)
    tags, starts, _ = genome(n_genes, step)
    rows = []
    for k in range(n):
        base = (0, 12, 24)[k % 3]
        a, b = base + int(rng.integers(0, 3)), base + 3 + int(rng.integers(0, 3))
        p1 = starts[a] + int(rng.integers(0, 900))
        rows.append(dict(pos1=p1, pos2=starts[b] + int(rng.integers(0, 900)), MI=float(rng.random()), srp=float(rng.random() * 6), pos1_genreg=tags[a], pos2_genreg=tags[b]))
    order = rng.permutation(n)
    return pd.DataFrame([rows[i] for i in order])


# ---- segments ----------------------------------------------------------------------------------------------------------------------------------

def test_segments_equal_scipy_where_distances_are_distinct():
    rng = np.random.default_rng(20)
    for trial in range(60):
        n = int(rng.integers(5, 41))
        while True:
            v = rng.choice(10 ** 7, n, replace=False).astype(np.float64)
            d = np.abs(v[:, None] - v[None, :])[np.triu_indices(n, 1)]
            if len(np.unique(d)) == len(d):
                break
        assert len(np.unique(d)) == len(d)
        Z = linkage(v[:, None], "complete")
        for k in (1, 2, 5, n):
            want = TR.cutree_labels(fcluster(Z, k, "maxclust").tolist())
            assert np.array_equal(T.complete_linkage_1d(v, k), want), (trial, k)


def test_segments_equal_the_brute_force_under_ties():
    rng = np.random.default_rng(21)
    for trial in range(40):
        n = int(rng.integers(2, 14))
        v = rng.integers(0, 6, n).astype(np.float64) * 10          # repeats and equal gaps everywhere
        for k in range(1, n + 1):
            assert np.array_equal(T.complete_linkage_1d(v, k), TR.brute_complete_linkage(v, k)), (v, k)


def test_relabelling_is_the_permutation_itself():
    # first-appearing cluster rightmost, second leftmost, third in the middle: ord = (2, 3, 1), a 3-cycle
    pos1 = [900, 910, 100, 110, 500, 510]
    seg, rank = T.tanglegram_segments(pos1, 3)
    assert seg.tolist() == [2, 2, 3, 3, 1, 1]
    left_to_right = [int(seg[i]) for i in np.argsort(pos1)][::2]
    assert left_to_right == [3, 1, 2]                                # tng_2 is NOT the second stretch from the left
    assert rank.tolist() == [2, 3, 1]
    # where ord is an involution the files are numbered from the left
    seg, rank = T.tanglegram_segments([500, 510, 100, 110, 900, 910], 3)
    assert seg.tolist() == [2, 2, 1, 1, 3, 3] and rank.tolist() == [1, 2, 3]


def test_segments_match_the_transliteration():
    th = make_tophits()
    seg, _ = T.tanglegram_segments(th["pos1"], 3)
    ref = TR.reference(th, 3, "SR", cds=record(*genome()).cds)
    for r in ref:
        assert len(r["links"]) > 0
    got = T.create_tanglegram(th, gbk=record(*genome()), break_segments=3)
    assert [g["segment"] for g in got] == [1, 2, 3] and sorted(g["rank"] for g in got) == [1, 2, 3]
    for g, r in zip(got, ref):
        for key in ("chr", "ann", "links"):
            pd.testing.assert_frame_equal(g[key], r[key], check_exact=True)
        assert (seg == g["segment"]).sum() > 0


# ---- links -----------------------------------------------------------------------------------------------------------------------------------------

def test_links_take_the_maximum_weight_per_pair():
    p1 = ["b", "a", "b", "a", "Z", "b"]
    p2 = ["x", "x", "x", "b", "a", "y"]
    w = [1.0, 5.0, 3.0, 2.0, 9.0, 0.5]
    u1, u2, uw, locs = T.tanglegram_links(p1, p2, w)
    assert list(zip(u1, u2)) == [("Z", "a"), ("a", "b"), ("a", "x"), ("b", "x"), ("b", "y")]      # code-point order: "Z" < "a"
    assert uw.tolist() == [9.0, 2.0, 5.0, 3.0, 0.5]
    assert locs == ["Z", "a", "b", "x", "y"]                          # p1a's distinct names, then p2a's new ones


def test_links_drop_rows_without_a_name():
    with pytest.warns(UserWarning, match="2 rows without a gene region name"):
        u1, u2, uw, locs = T.tanglegram_links(["a", None, "c", "d"], ["x", "y", "", "z"], [1.0, 2.0, 3.0, 4.0])
    assert list(zip(u1, u2)) == [("a", "x"), ("d", "z")] and uw.tolist() == [1.0, 4.0]
    with pytest.warns(UserWarning):
        assert T.tanglegram_links([float("nan")], ["x"], [1.0])[3] == []


def test_lr_takes_mi():
    th = make_tophits()
    rec = record(*genome())
    sr = T.create_tanglegram(th, gbk=rec, break_segments=3, links_type="SR")
    lr = T.create_tanglegram(th, gbk=rec, break_segments=3, links_type="LR")
    ref = TR.reference(th, 3, "LR", cds=rec.cds)
    for a, b, r in zip(sr, lr, ref):
        pd.testing.assert_frame_equal(b["links"], r["links"], check_exact=True)
        assert a["links"]["V1"].tolist() == b["links"]["V1"].tolist() and not np.array_equal(a["links"]["w"], b["links"]["w"])
        assert b["links"]["w"].max() <= th["MI"].max()


# ---- lookup ----------------------------------------------------------------------------------------------------------------------------------------

def test_lookup_first_match_wins():
    rec = record(["SP_0100", "SP_01", "SP_0100", "other"], [10, 200, 3000, 40000], [90, 290, 3090, 40090])
    rng, nf = T.locus_ranges(["SP_0100", "SP_01", "other"], gbk=rec)
    assert nf == [] and rng == [(10, 90), (10, 90), (40000, 40090)]      # "SP_01" lies inside the earlier tag "SP_0100": that row's own start and end
    assert T.locus_ranges(["SP_01"], gbk={"gbk": rec, "ref_g": 0})[0] == [(10, 90)]
    rec2 = record(["SP_01", "SP_0100"], [200, 10], [290, 90])
    assert T.locus_ranges(["SP_01", "SP_0100"], gbk=rec2)[0] == [(200, 290), (10, 90)]     # a name that is a substring of a LATER tag finds its own row first


def test_lookup_strips_gene_for_gff_only():
    ann = annotation(["ID=cds1;locus_tag=abc", "ID=77_5;Name=x"], [100, 2000], [400, 2600])
    rng, nf = T.locus_ranges(["GENE_77_5", "abc", "GENE_GENE_cds1"], gff=ann)
    assert nf == [] and rng == [(2000, 2600), (100, 400), (100, 400)]
    rec = record(["77_5"], [2000], [2600])
    with pytest.warns(UserWarning, match="Could not locate GENE_77_5 in the genbankr parsed gbk file, these link will be dropped from the tanglegram..."):
        rng, nf = T.locus_ranges(["GENE_77_5"], gbk=rec)
    assert nf == ["GENE_77_5"] and rng == [None]


def test_lookup_is_literal():
    rec = record(["a.c", "abc"], [1, 100], [50, 150])
    assert T.locus_ranges(["a.c"], gbk=rec)[0] == [(1, 50)]
    with pytest.warns(UserWarning):
        assert T.locus_ranges(["a.*"], gbk=rec)[1] == ["a.*"]


@pytest.mark.parametrize("kind", ["gbk", "gff"])
def test_intergenic_names_are_dropped_with_their_pairs(kind):
    tags, starts, ends = genome(12)
    src = dict(gbk=record(tags, starts, ends)) if kind == "gbk" else dict(gff=annotation([f"ID={t}" for t in tags], starts, ends))
    th = pd.DataFrame({"pos1": [1100, 1200, 5100, 9100, 40000, 40100], "pos1_genreg": ["G000", "G000-G001", "G001", "G002", "G009-G010", "G009-G010"],
                       "pos2_genreg": ["G001", "G002", "G000-G001", "G003", "G010", "G011"], "srp": [1.0, 2.0, 3.0, 4.0, 5.0, 6.0], "MI": [0.1] * 6})
    with warnings.catch_warnings(record=True) as rec_w:
        warnings.simplefilter("always")
        got = T.create_tanglegram(th, break_segments=2, **src)
    msgs = [str(w.message) for w in rec_w]
    assert any(m.startswith("Could not locate G000-G001 in the genbankr parsed gbk file") for m in msgs)
    assert any(m.startswith("Could not locate G009-G010 in") for m in msgs)
    assert any("Tanglegram 2 has no link left" in m for m in msgs)
    a, b = got
    assert a["links"]["V1"].tolist() == ["p_G000", "p_G002"] and a["links"]["V3"].tolist() == ["q_G001", "q_G003"] and a["links"]["w"].tolist() == [1.0, 4.0]
    assert a["ann"]["V1"].tolist() == ["p_G000", "p_G002", "p_G001", "p_G003", "q_G000", "q_G002", "q_G001", "q_G003"]      # all_locs recomputed; every locus on both bars
    assert a["chr"]["V2"].tolist() == [0, 0] and a["chr"]["V3"].tolist() == [starts[3] + 899 + 1000] * 2
    assert len(b["links"]) == 0 and len(b["ann"]) == 0 and len(b["chr"]) == 0 and len(b["capsules"]) == 0 and len(b["rects"]) == 0 and "png" not in b
    ref = TR.reference(th, 2, "SR", cds=src["gbk"].cds if kind == "gbk" else None, gff=src["gff"].gff if kind == "gff" else None)
    for key in ("chr", "ann", "links"):
        pd.testing.assert_frame_equal(a[key], ref[0][key], check_exact=True)
    assert ref[1]["links"] is None


# ---- layout and marks ---------------------------------------------------------------------------------------------------------------------------------

def test_layout_rules():
    W, H = 1000, 600
    locs = ["wide", "tiny", "near", "far"]
    ranges = [(2000, 5000), (10000, 10001), (10030, 10040), (60000, 61000)]
    v2, v3 = 1000, 62000
    lay = T.tanglegram_layout(v2, v3, locs, ranges, W, H, 4)
    s, mx, pw = lay["s"], lay["mx"], lay["PW"]
    assert (s, mx, pw) == (N.text_scale(W), W // 20, W - 2 * (W // 20))

    def x(c):
        return mx + ((c - v2) * (pw - 1)) // (v3 - v2)

    assert x(v2) == mx and x(v3) == mx + pw - 1
    assert lay["x0"].tolist() == [x(a) for a, _ in ranges] and lay["x1"].tolist() == [x(b) + 1 for _, b in ranges]
    assert lay["x1"][1] - lay["x0"][1] == 1                            # a locus shorter than a pixel is one pixel wide
    assert lay["xc"].tolist() == [(x(a) + x(b)) // 2 for a, b in ranges]
    lmax = (6 * 4 - 1) * s
    assert lay["yp"] == 24 * s + lmax and lay["yq"] == H - 18 * s - lmax and lay["bar_h"] == 12 * s
    # "tiny" and "near" are closer than a label's width: the first by (xc, index) is drawn, the other gets a box with w = 0
    assert abs(int(lay["xc"][1]) - int(lay["xc"][2])) < 7 * s
    assert lay["drawn"].tolist() == [True, True, False, True]
    n = len(locs)
    for i in range(n):
        lx = int(lay["xc"][i]) - (7 * s) // 2
        p, q = lay["label_box"][i].tolist(), lay["label_box"][n + i].tolist()
        if lay["drawn"][i]:
            tw = (6 * len(locs[i]) - 1) * s
            assert p == [lx, lay["yp"] - 2 * s - tw, 7 * s, tw] and q == [lx, lay["yq"] + 14 * s, 7 * s, tw]
            assert p[1] >= 22 * s and q[1] + q[3] <= H - 4 * s
        else:
            assert p[2] == 0 and q[2] == 0
    assert lay["title"] == "Tanglegram 4: 1000 - 62000 bp"
    # drawn labels keep s free columns between them
    xs = sorted(int(lay["label_box"][i][0]) for i in range(n) if lay["drawn"][i])
    assert all(b - (a + 7 * s) >= s for a, b in zip(xs, xs[1:]))


def test_layout_refusals():
    with pytest.raises(ValueError, match="between the bars"):
        T.tanglegram_layout(0, 10000, ["abcdefghij"], [(1000, 2000)], 640, 200)      # 2 x (59 + 12) + 42 + 64 > 200
    T.tanglegram_layout(0, 10000, ["abcdefghij"], [(1000, 2000)], 640, 24 + 59 + 12 + 64 + 18 + 59)
    with pytest.raises(ValueError, match="between the bars"):
        T.tanglegram_layout(0, 10000, ["abcdefghij"], [(1000, 2000)], 640, 24 + 59 + 12 + 63 + 18 + 59)
    for w, h in ((63, 400), (8193, 400), (640, 63), (640, 8193)):
        with pytest.raises(ValueError, match="64..8192"):
            T.tanglegram_layout(0, 10000, ["a"], [(1000, 2000)], w, h)


def test_marks():
    W, H = 1000, 600
    locs = ["a", "b", "c"]
    ranges = [(2000, 5000), (20000, 23000), (50000, 52000)]
    lay = T.tanglegram_layout(1000, 62000, locs, ranges, W, H)
    p1a, p2a, w = ["a", "a", "b"], ["b", "c", "c"], np.asarray([2.0, 8.0, float("nan")])
    caps, rects = T.tanglegram_marks(lay, p1a, p2a, w, locs)
    s, yp, yq = lay["s"], lay["yp"], lay["yq"]
    assert rects[["x0", "y0", "x1", "y1", "rgb"]].tolist()[:2] == [(50, yp, 950, yp + 12 * s, T.RGB_BAR), (50, yq, 950, yq + 12 * s, T.RGB_BAR)]
    assert rects["rgb"].tolist()[2:] == [T.RGB_LOCUS] * 6 and rects["y0"].tolist()[2:] == [yp] * 3 + [yq] * 3
    assert rects["x0"].tolist()[2:5] == lay["x0"].tolist() and rects["x1"].tolist()[5:] == lay["x1"].tolist()
    assert len(caps) == 3 * N.ARC_SEGMENTS
    # non-finite weights count as 0 and NaN makes the maximum NaN: every w' is 0 here, ties in pair order
    assert set(caps["w"].tolist()) == {1} and set(caps["alpha"].tolist()) == {64}
    w = np.asarray([2.0, 8.0, 4.0])
    caps, _ = T.tanglegram_marks(lay, p1a, p2a, w, locs)
    links = caps.reshape(3, N.ARC_SEGMENTS)
    assert links["alpha"][:, 0].tolist() == [112, 160, 255] and links["w"][:, 0].tolist() == [2, 2, 3]       # ascending weight: the strongest link last
    assert (caps["rgb"] == T.RGB_LINK).all()
    xc = lay["xc"]
    ends = [((int(l["x0"][0]), int(l["y0"][0])), (int(l["x1"][-1]), int(l["y1"][-1]))) for l in links]
    assert ends == [((xc[0], yp + 12 * s), (xc[1], yq - 1)), ((xc[1], yp + 12 * s), (xc[2], yq - 1)), ((xc[0], yp + 12 * s), (xc[2], yq - 1))]
    for l in links:                                                    # a connected polyline that goes down all the way
        assert l["x1"][:-1].tolist() == l["x0"][1:].tolist() and l["y1"][:-1].tolist() == l["y0"][1:].tolist()
        assert (np.diff(l["y0"]) > 0).all()
    mid = T.link_polyline((100, 100), (400, 400))[N.ARC_SEGMENTS // 2]
    assert mid.tolist() == [250, 250]                                  # the curve's midpoint: halfway, by symmetry


# ---- the stage function ----------------------------------------------------------------------------------------------------------------------------------

def test_refusals():
    th = make_tophits()
    rec, ann = record(*genome()), annotation([f"ID={t}" for t in genome()[0]], *genome()[1:])
    with pytest.raises(ValueError, match="Provide either one of gbk or gff"):
        T.create_tanglegram(th)
    with pytest.raises(ValueError, match="Provide either one of gbk or gff"):
        T.create_tanglegram(th, gbk=rec, gff=ann)
    with pytest.raises(ValueError, match="Links type must be SR or LR"):
        T.create_tanglegram(th, gbk=rec, links_type="sr")
    with pytest.raises(ValueError, match="at least 2 rows"):
        T.create_tanglegram(th.iloc[:1], gbk=rec, break_segments=1)
    for k in (0, 11, -1, 2.5):
        with pytest.raises(ValueError, match="1..10"):
            T.create_tanglegram(th, gbk=rec, break_segments=k)
    with pytest.raises(ValueError, match="5 segments for 4 rows"):
        T.create_tanglegram(th.iloc[:4], gbk=rec, break_segments=5)
    with pytest.raises(ValueError, match="64..8192"):
        T.create_tanglegram(th, gbk=rec, break_segments=3, plot_w=10)
    with pytest.raises(ValueError, match="between the bars"):
        T.create_tanglegram(th, gbk=rec, break_segments=3, plot_w=640, plot_h=100)


def test_entry_resolves_and_needs_no_gpu_without_a_folder(monkeypatch):
    assert ldweaver_amd.create_tanglegram is T.create_tanglegram and "create_tanglegram" in ldweaver_amd.__all__
    from ldweaver_amd import engine as E

    def no_gpu(self, *a, **k):
        raise AssertionError("an Engine was made")

    monkeypatch.setattr(E.Engine, "__init__", no_gpu)
    got = T.create_tanglegram(make_tophits(), gff=annotation([f"ID={t};x" for t in genome()[0]], *genome()[1:]), break_segments=3, plot_w=640, plot_h=400)
    assert len(got) == 3
    for g in got:
        assert "png" not in g and "boxes" not in g and len(g["capsules"]) == len(g["links"]) * N.ARC_SEGMENTS and len(g["rects"]) == 2 + len(g["ann"])
        assert g["capsules"].dtype == E.Engine.CAPSULE and g["rects"].dtype == E.Engine.RECT
        assert set(g) >= {"segment", "rank", "chr", "ann", "links", "capsules", "rects", "labels"}
