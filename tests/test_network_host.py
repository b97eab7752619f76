"""CPU: ldweaver_amd.network against the literal restatement of R/createNetworkPlot.R in tests/network_ref.py — create_network's edge list
(:36-118), the layout's own properties, and create_network_for_gene through its pandas route (:169-290)."""
import numpy as np
import pandas as pd
import pytest

import network_ref as NR
from ldweaver_amd import network as N


def _hits(pairs, mi=None):
    mi = np.linspace(0.9, 0.1, len(pairs)) if mi is None else mi
    return pd.DataFrame({"pos1_ann": [a for a, _ in pairs], "pos2_ann": [b for _, b in pairs], "MI": mi})


def _same_edges(t, **kw):
    got, want = N.network_edges(t, **kw), NR.edges(t, **kw)
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    return got


CRAFTED = [("geneA:x", "geneB:y"), ("geneB:1", "geneA:2"), ("geneA:q", "geneB:z"), ("geneB:7", "geneC:1"), ("geneC:2", "geneB:3"), ("geneD:1", "geneD:2"),
           ("geneD:3", "geneD:4"), ("geneE:1", "geneF:1"), ("geneA:x", "geneB:y"), ("lonely", "geneA:9"), ("lonely", "geneA:8"), ("geneB:7", "geneC:1")]


def test_edges_merge_of_reversed_pairs():
    """(geneA, geneB) x3 and (geneB, geneA) x1 become one edge with the counts summed and the larger weight."""
    t = _hits(CRAFTED, mi=np.array([.2, .7, .1, .3, .4, .9, .8, .05, .25, .5, .6, .35]))
    e = _same_edges(t, min_links_to_include=1)
    ab = e[(e.p1.isin(["geneA", "geneB"])) & (e.p2.isin(["geneA", "geneB"]))]
    la = e[(e.p1.isin(["lonely", "geneA"])) & (e.p2.isin(["lonely", "geneA"]))]
    assert len(ab) == 1 and int(ab.Num_Links.iloc[0]) == 4 and len(la) == 1 and int(la.Num_Links.iloc[0]) == 2
    assert np.isclose(ab.weights.iloc[0] / la.weights.iloc[0], 0.7 / 0.6)
    assert not (e.p1 == e.p2).any() and e.weights.max() == 1.0
    assert "geneD" not in set(e.p1) | set(e.p2)            # a loop only


def test_edges_both_swap_passes():
    """geneB is p1a in one pair and p2a in another: pass one swaps it to the right, pass two swaps what then sits on both sides."""
    _same_edges(_hits([("b:1", "c:1"), ("a:1", "b:1"), ("c:1", "d:1"), ("d:2", "a:2")]), min_links_to_include=1)
    _same_edges(_hits(CRAFTED), min_links_to_include=2)


def test_edges_only_loops_and_below_the_cut():
    with pytest.raises(ValueError, match="Everything is a loop"):
        N.network_edges(_hits([("g:1", "g:2"), ("g:3", "g:4"), ("h", "h")]), min_links_to_include=1)
    with pytest.raises(ValueError, match="Everything is a loop"):
        NR.edges(_hits([("g:1", "g:2"), ("g:3", "g:4"), ("h", "h")]), min_links_to_include=1)
    e = _same_edges(_hits(CRAFTED), min_links_to_include=2)
    assert "geneE" not in set(e.p1) | set(e.p2)            # one link only: below min_links_to_include


@pytest.mark.parametrize("max_nodes", [2, 3, 6, 7, 40])
def test_edges_max_plot_nodes(max_nodes):
    """CRAFTED has 7 distinct ordered pairs: fewer, as many, and more nodes asked for (40 is also past the last row)."""
    assert len({(a.split(":")[0], b.split(":")[0]) for a, b in CRAFTED}) == 7
    _same_edges(_hits(CRAFTED), max_plot_nodes=max_nodes, min_links_to_include=1)


def test_edges_separator():
    t = _hits([("a|1", "b|2"), ("a|3", "b|4"), ("nosep", "b|1"), ("nosep", "b|9"), ("a:1", "a:2"), ("a:1", "a:2")])
    e = _same_edges(t, separator="|", min_links_to_include=2)
    assert set(e.p1) | set(e.p2) == {"a", "b", "nosep", "a:1", "a:2"}
    e = _same_edges(t, separator=":", min_links_to_include=1)       # no ':' in most annotations: the whole string is the node
    assert "nosep" in set(e.p1) | set(e.p2)


def _graph(sizes):
    """components that are paths of the given node counts"""
    p1, p2, k = [], [], 0
    for m in sizes:
        for j in range(m - 1):
            p1.append(f"n{k + j}")
            p2.append(f"n{k + j + 1}")
        k += m
    return pd.DataFrame({"p1": p1, "p2": p2, "Num_Links": np.arange(len(p1)) % 3 + 1, "weights": np.linspace(0.1, 1.0, len(p1))})


@pytest.mark.parametrize("w,h", [(6000, 4000), (600, 400), (333, 777)])
def test_layout_properties(w, h):
    e = _graph([3, 40, 2, 2, 5])
    names, xy, comp = N.network_layout(e, w, h)
    assert len(names) == 52 and names[0] == "n0" and xy.dtype == np.int32
    assert (xy[:, 0] >= 0).all() and (xy[:, 0] < w).all() and (xy[:, 1] >= 0).all() and (xy[:, 1] < h).all()
    assert len({tuple(p) for p in xy.tolist()}) == 52                       # distinct nodes, distinct pixels
    names2, xy2, comp2 = N.network_layout(e, w, h)
    assert names2 == names and np.array_equal(xy, xy2) and np.array_equal(comp, comp2)
    assert comp[names.index("n3")] == 0 and comp[names.index("n47")] == 1   # 40 nodes first, then 5, 3, and the two pairs by first appearance
    assert comp[names.index("n0")] == 2 and comp[names.index("n43")] == 3 and comp[names.index("n45")] == 4
    pair = [xy[names.index("n43")], xy[names.index("n44")]]                 # a one-edge component: a horizontal line
    assert pair[0][1] == pair[1][1] and pair[0][0] < pair[1][0]
    caps, levels, pal = N.network_capsules(e, names, xy, w)
    assert len(caps) == 16 * len(e) and levels == [1, 2, 3] and pal == N.hue_palette(3)
    assert caps["w"].min() >= 1 and caps["alpha"].min() >= 1 and caps["alpha"].max() <= 255
    first = caps[:16]                                                       # an edge's polyline is connected and ends on its nodes
    assert (first["x0"][0], first["y0"][0]) == tuple(xy[0]) and (first["x1"][-1], first["y1"][-1]) == tuple(xy[1])
    assert np.array_equal(first["x1"][:-1], first["x0"][1:]) and np.array_equal(first["y1"][:-1], first["y0"][1:])


def test_hue_palette_is_ggplot2s():
    assert N.hue_palette(3) == [0xF8766D, 0x00BA38, 0x619CFF] and N.hue_palette(1) == [0xF8766D]
    assert N.hue_palette(4) == [0xF8766D, 0x7CAE00, 0x00BFC4, 0xC77CFF]


def test_create_network_without_a_path_needs_no_gpu():
    r = N.create_network(_hits(CRAFTED), plot_w=600, plot_h=400)
    assert list(r["edges"].columns) == ["p1", "p2", "Num_Links", "weights"] and "png" not in r
    assert r["nodes"] == list(dict.fromkeys(x for a, b in zip(r["edges"].p1, r["edges"].p2) for x in (a, b)))
    with pytest.raises(ValueError):
        N.create_network(_hits(CRAFTED), plot_w=10, plot_h=400)


# ---- create_network_for_gene, pandas route ------------------------------------------------------------------------------------------------

SR_COLS = ("pos1", "pos2", "len", "ARACNE", "MI", "srp", "pos1_ann", "pos2_ann", "pos1_genreg", "pos2_genreg", "links", "pos1_ad", "pos2_ad")
LR_COLS = ("pos1", "pos2", "len", "ARACNE", "MI", "pos1_ann", "pos2_ann", "pos1_genreg", "pos2_genreg", "links", "pos1_ad", "pos2_ad")


def write_annotated(path, cols, rows):
    with open(path, "w") as fh:
        fh.write("\t".join(cols) + "\n")
        for r in rows:
            fh.write("\t".join(str(r[c]) for c in cols) + "\n")


def gene_files(tmp_path, n=300, seed=5):
    """An sr and an lr file over the same few genes; the lr file repeats some sr rows exactly (duplicated() must drop them)."""
    rng = np.random.default_rng(seed)
    genes = ["pbp2x", "pbp2xL", "pbp1a", "dnaA", "gyrB", "parC", "folA", "rpoB", "murM", "x"]
    links = ["syXsy", "nsXsy", "syXns", "nsXns", "syXsyX"]

    def row(k):
        a, b = rng.choice(len(genes), 2, p=[.25, .05, .2, .1, .1, .1, .05, .05, .05, .05])
        p1 = int(rng.integers(1, 200000))
        return dict(pos1=p1, pos2=p1 + int(rng.integers(1, 5000)), len=int(rng.integers(1, 5000)), ARACNE=int(rng.random() < 0.7), MI=round(float(rng.random()), 6),
                    srp=round(float(rng.random() * 9), 4), pos1_ann=f"{genes[a]}:{rng.integers(1, 900)}:A>T", pos2_ann=f"{genes[b]}:{rng.integers(1, 900)}:C>G",
                    pos1_genreg=f"reg_{genes[(a + 3) % 10]}", pos2_genreg="pbp2x_region", links=str(rng.choice(links)), pos1_ad="A:0.5", pos2_ad="C:0.5")
    sr = [row(k) for k in range(n)]
    lr = [row(k) for k in range(n)]
    lr[10:10] = [sr[3], sr[4], sr[5]]
    write_annotated(tmp_path / "sr.tsv", SR_COLS, sr)
    write_annotated(tmp_path / "lr.tsv", LR_COLS, lr)
    return str(tmp_path / "sr.tsv"), str(tmp_path / "lr.tsv")


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("gene", ["pbp2x", "pbp1a", "pbp", "absent"])
def test_for_gene_pandas_route(tmp_path, gene, level):
    """"pbp" matches as a substring only, so at level 2 R's genes[-which(genes == gene_name)] empties the gene list: level 2 adds nothing."""
    sr, lr = gene_files(tmp_path)
    for kw in (dict(), dict(drop_syXsy=False, drop_indirect=False), dict(min_links_to_include=1)):
        got = N.create_network_for_gene(gene, sr, lr, level=level, reader="pandas", **kw)
        want = NR.for_gene(gene, sr, lr, level=level, **kw)
        assert list(got.columns) == NR.FRAME_COLS
        if len(want) == 0:
            assert len(got) == 0
            continue
        pd.testing.assert_frame_equal(got, want, check_exact=True)
        assert not got.duplicated().any()
    one = N.create_network_for_gene(gene, sr, None, level=level, reader="pandas")
    assert len(one) <= len(N.create_network_for_gene(gene, sr, lr, level=level, reader="pandas"))
    if gene == "pbp" and level == 2:
        l1 = N.create_network_for_gene(gene, sr, lr, level=1, reader="pandas")
        pd.testing.assert_frame_equal(N.create_network_for_gene(gene, sr, lr, level=2, reader="pandas"), l1)
    if gene == "pbp2x" and level == 2:
        assert len(got) > len(N.create_network_for_gene(gene, sr, lr, level=1, reader="pandas", min_links_to_include=1))


def test_for_gene_argument_checks():
    with pytest.raises(ValueError, match="must be provided"):
        N.create_network_for_gene("g")
    with pytest.raises(ValueError, match="Level must be 1 or 2"):
        N.create_network_for_gene("g", "a.tsv", level=3)
    with pytest.raises(ValueError, match="reader"):
        N.create_network_for_gene("g", "a.tsv", reader="fast")
