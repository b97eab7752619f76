"""CPU: the host side of the tree view (ldweaver_amd/tree.py) against the naive counterparts of tests/tree_ref.py — the Newick parser, midpoint
rooting, ladderizing, the reference's selection of links, columns, FASTA rows and metadata rows, and the layout."""
import warnings

import numpy as np
import pandas as pd
import pytest

import tree_ref as TR
from ldweaver_amd import tree as T


def _tip_sets(tree):
    """Per node the frozenset of tip labels below it."""
    sets = [set() for _ in range(tree.n_nodes)]
    for t, v in enumerate(tree.tip_node):
        sets[v].add(tree.tip_label[t])
    for v in range(tree.n_nodes - 1, 0, -1):
        sets[tree.parent[v]] |= sets[v]
    return [frozenset(s) for s in sets]


def random_newick(rng, n_tips, zero_frac=0.1):
    """A random tree of n_tips tips t0.. with multifurcations, as Newick text (tips named in file order)."""
    items = [f"t{k}" for k in range(n_tips)]
    rng.shuffle(items)

    def ln():
        return 0.0 if rng.random() < zero_frac else round(float(rng.random() * 3), 4)

    items = [f"{s}:{ln()}" for s in items]
    while len(items) > 1:
        k = min(len(items), int(rng.integers(2, 5)))
        if len(items) <= 3:
            k = len(items)
        pick = sorted(rng.choice(len(items), k, replace=False).tolist(), reverse=True)
        grp = [items.pop(j) for j in pick]
        items.append("(" + ",".join(grp) + ")" + (f":{ln()}" if items else ""))
    return items[0] + ";"


# ---- the parser -------------------------------------------------------------------------------------------------------------------------------------------

def test_parser_grammar():
    text = b"[a comment] ( 'it''s A':1.5e-1 , B_b [inner] : 2E+1, (C,D:.5)inner:3, 'x y(z)' :1 )root ; (ignored);"
    t = T.parse_newick(text)
    assert t.tip_label == ["it's A", "B_b", "C", "D", "x y(z)"]
    assert t.n_nodes == 7 and t.parent.tolist() == [-1, 0, 0, 0, 3, 3, 0]
    assert t.length.tolist() == [0.0, 0.15, 20.0, 3.0, 0.0, 0.5, 1.0]
    assert t.tip_node.tolist() == [1, 2, 4, 5, 6]
    assert t.children(0).tolist() == [1, 2, 3, 6] and t.children(3).tolist() == [4, 5] and t.children(1).tolist() == []
    assert t.tip_order().tolist() == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("text,offset,what", [
    (b"(A,B", 4, "ends"),
    (b"(A,B));", 5, r"'\)' without"),
    (b"(A,B;", 4, "open"),
    (b"(A:x,B);", 3, "branch length"),
    (b"(A,,B);", 3, "without a label"),
    (b"(A B);", 3, "unexpected character"),
    (b"(A,'B);", 3, "quoted label"),
    (b"(A,B)[c;", 5, "comment"),
    (b"A,B;", 1, "outside"),
])
def test_parser_errors_name_the_offset(text, offset, what):
    with pytest.raises(ValueError, match=what) as e:
        T.parse_newick(text)
    assert f"byte {offset}" in str(e.value)


def test_parser_refuses_one_tip_and_duplicates():
    with pytest.raises(ValueError, match="at least two"):
        T.parse_newick(b"(A);")
    with pytest.raises(ValueError, match="more than once"):
        T.parse_newick(b"(A,(B,A));")


def test_caterpillar_of_70000_tips_parses(tmp_path):
    n = 70000
    text = "(" * (n - 1) + "t0:1" + "".join(f",t{k}:1):0.5" for k in range(1, n))
    text = text[:text.rindex(":")] + ";"
    p = tmp_path / "cat.nwk"
    p.write_text(text)
    t = T.read_newick(p)
    assert t.n_tips == n and t.n_nodes == 2 * n - 1 and t.tip_label[-1] == f"t{n - 1}"
    assert int(t.tip_node[0]) == n - 1      # n - 1 nested parentheses above the first tip
    r = T.ladderize(T.midpoint_root(t))
    assert r.n_tips == n and sorted(r.tip_order().tolist()) == list(range(n))


@pytest.mark.parametrize("seed", range(12))
def test_parser_matches_the_recursive_reader(seed):
    rng = np.random.default_rng(seed)
    text = random_newick(rng, int(rng.integers(2, 61)))
    t = T.parse_newick(text.encode())
    ref = TR.newick(text)
    assert t.tip_label == TR.node_tips(ref)
    got, want = TR.array_distances(t.parent, t.length, t.tip_node, t.tip_label), TR.node_distances(ref)
    assert got.keys() == want.keys()
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-12, abs=0)


# ---- rooting ---------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(40))
def test_midpoint_root_on_random_trees(seed):
    rng = np.random.default_rng(1000 + seed)
    n = [2, 3, 4, 60][seed] if seed < 4 else int(rng.integers(2, 61))
    text = random_newick(rng, n)
    want = TR.node_distances(TR.newick(text))
    if max(want.values()) == 0:      # (every length drawn as zero: draw again without zeros)
        text = random_newick(rng, n, zero_frac=0.0)
        want = TR.node_distances(TR.newick(text))
    t = T.parse_newick(text.encode())
    r = T.midpoint_root(t)
    assert r.tip_label == t.tip_label and np.all(r.parent[1:] < np.arange(1, r.n_nodes)) and r.parent[0] == -1
    got = TR.array_distances(r.parent, r.length, r.tip_node, r.tip_label)
    scale = max(want.values())
    for k in want:      # every tip-to-tip distance is unchanged
        assert abs(got[k] - want[k]) <= 1e-12 * scale, (k, got[k], want[k])
    # the two most distant tips sit on different sides of the root, equally deep
    a, b = max(want, key=lambda k: want[k])
    depth = TR.array_depths(r.parent, r.length)
    sets = _tip_sets(r)
    side = {lab: c for c in r.children(0) for lab in sets[c]}
    assert side[a] != side[b]
    da, db = depth[r.tip_node[r.tip_label.index(a)]], depth[r.tip_node[r.tip_label.index(b)]]
    assert abs(da - db) <= 1e-12 * scale and abs(da + db - want[(a, b)]) <= 1e-12 * scale
    assert max(depth) <= da + 1e-12 * scale
    assert r.n_nodes <= t.n_nodes + 1


def test_root_on_a_node_adds_no_node():
    t = T.parse_newick(b"((A:3,B:1):2,C:1,D:1);")       # C .. A = 6, half way = the node above A and B
    r = T.midpoint_root(t)
    assert r.n_nodes == t.n_nodes == 6
    sets = _tip_sets(r)
    assert [sorted(sets[c]) for c in r.children(0)] == [["A"], ["B"], ["C", "D"]]      # the old parent comes last
    assert r.length[r.children(0)].tolist() == [3.0, 1.0, 2.0]
    t = T.parse_newick(b"(A:2,B:2,C:1);")               # the root it has
    assert T.midpoint_root(t).n_nodes == 4


def test_split_branch_and_old_root_removed():
    t = T.parse_newick(b"((A:1,B:1):1,(C:1,D:5):1);")   # D .. A = 8: the root goes 4 from D on D's branch; the old root is left with two branches
    r = T.midpoint_root(t)
    assert r.n_nodes == 7
    sets = _tip_sets(r)
    kids = r.children(0).tolist()
    assert [sorted(sets[c]) for c in kids] == [["D"], ["A", "B", "C"]] and r.length[kids].tolist() == [4.0, 1.0]
    inner = kids[1]
    assert [sorted(sets[c]) for c in r.children(inner)] == [["C"], ["A", "B"]] and r.length[r.children(inner)].tolist() == [1.0, 2.0]
    t = T.parse_newick(b"((A:1,B:3):1,C:1,D:1);")       # B .. C = 5: a new node 2.5 from B; the old root keeps its three branches
    assert T.midpoint_root(t).n_nodes == t.n_nodes + 1


def test_tie_rule_and_refusals():
    t = T.parse_newick(b"(A:1,B:1,C:1,D:1);")
    a, b, _ = T.diameter_tips(t)
    assert (a, b) == (1, 0)      # farthest from tip 0: B, C, D tie -> B; farthest from B: A, C, D tie -> A
    t = T.parse_newick(b"(A:1,(B:2,C:2):1,D:3);")
    a, b, _ = T.diameter_tips(t)
    assert (a, b) == (1, 3)      # from A: B, C, D at 4 -> B; from B: D at 6
    with pytest.raises(ValueError, match="negative"):
        T.midpoint_root(T.parse_newick(b"(A:1,B:-1);"))
    with pytest.raises(ValueError, match="zero"):
        T.midpoint_root(T.parse_newick(b"(A,B,(C,D));"))


# ---- ladderize -----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(10))
def test_ladderize(seed):
    rng = np.random.default_rng(2000 + seed)
    t = T.parse_newick(random_newick(rng, int(rng.integers(2, 61))).encode())
    lad = T.ladderize(t)
    before, after = _tip_sets(t), _tip_sets(lad)
    want = {before[v]: sorted((before[c] for c in t.children(v)), key=len) for v in range(t.n_nodes)}     # sorted() is stable
    assert len(after) == len(before)
    for v in range(lad.n_nodes):
        assert [after[c] for c in lad.children(v)] == want[after[v]]
    assert lad.tip_label == t.tip_label
    assert TR.array_distances(lad.parent, lad.length, lad.tip_node, lad.tip_label) == TR.array_distances(t.parent, t.length, t.tip_node, t.tip_label)
    order = lad.tip_order().tolist()
    assert sorted(order) == list(range(t.n_tips)) and [lad.tip_node[k] for k in order] == sorted(lad.tip_node.tolist())


# ---- the selection -----------------------------------------------------------------------------------------------------------------------------------------------------

TIPS = [f"iso{k}" for k in (3, 0, 4, 1, 2)]
POS = [101, 205, 330, 402, 517, 640, 700, 811]
COLS_LR = ["pos1", "pos2", "len", "MI", "ARACNE", "links"]
COLS_SR = ["pos1", "pos2", "len", "MI", "srp", "ARACNE", "links"]


def _tsv(path, cols, rows):
    path.write_text("\n".join(["\t".join(cols)] + ["\t".join(str(v) for v in r) for r in rows]) + "\n")
    return path


@pytest.fixture()
def files(tmp_path):
    rng = np.random.default_rng(5)
    names = ["extra1"] + [f"iso{k}" for k in range(5)] + ["extra2"]
    seqs = ["".join(rng.choice(list("ACGTNacgt-"), len(POS))) for _ in names]
    fa = tmp_path / "snps.fa"
    fa.write_text("".join(f">{n}\n{s}\n" for n, s in zip(names, seqs)))
    pos = tmp_path / "snps.pos"
    pos.write_text("".join(f"{p}\n" for p in POS))
    lr = [[101, 640, 539, 0.5, 1, "nsXns"], [205, 811, 606, 0.4, 1, "nsXsy"], [330, 700, 370, 0.3, 1, "nsXns"], [999, 640, 359, 0.2, 1, "nsXns"]]
    sr = [[402, 517, 115, 0.9, 4.5, 1, "nsXns"], [101, 205, 104, 0.8, 3.5, 1, "syXns"], [517, 640, 123, 0.7, 3.1, 1, "nsXns"]]
    d = dict(fasta=fa, pos=pos, names=names, seqs=seqs,
             lrt=_tsv(tmp_path / "lr_tophits.tsv", COLS_LR, lr[:3]), lra=_tsv(tmp_path / "lr_ann.tsv", COLS_LR, [lr[1], lr[3], lr[0]]),
             srt=_tsv(tmp_path / "sr_tophits.tsv", COLS_SR, sr[:2]), sra=_tsv(tmp_path / "sr_ann.tsv", COLS_SR, [sr[2], sr[0]]))
    return d


def _both(files, links_df=None, metadata=None, pos=None, fasta=None, tips=TIPS, which=("lrt", "lra", "srt", "sra"), **kw):
    """(ours, the transliteration's, our warnings) for one call."""
    paths = {k: (files[k] if k in which else None) for k in ("lrt", "lra", "srt", "sra")}
    pos_path, fa_path = pos or files["pos"], fasta or files["fasta"]
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = T.tree_selection(tips, metadata, fa_path, pos_path, links_df, paths["lrt"], paths["lra"], paths["srt"], paths["sra"],
                               kw.get("ntop_links", 10), kw.get("from_"), kw.get("to"))
    from ldweaver_amd.snpdat import read_fasta
    names, chars = read_fasta(str(fa_path))
    tabs = {k: (TR.read_table(v) if v is not None else None) for k, v in paths.items()}
    ref = TR.selection(tips, [float(s) for s in open(pos_path).read().split()], names, [bytes(r).decode() for r in chars],
                       links_df=None if links_df is None else (list(links_df.columns), links_df.values.tolist()),
                       lr_tophits=tabs["lrt"], lr_annotated=tabs["lra"], sr_tophits=tabs["srt"], sr_annotated=tabs["sra"],
                       metadata=None if metadata is None else (list(metadata.columns), metadata.values.tolist()),
                       ntop_links=kw.get("ntop_links", 10), frm=kw.get("from_"), to=kw.get("to"))
    return got, ref, [str(x.message) for x in w]


def _same(got, ref, msgs):
    assert got["pos_plot"] == ref["pos_plot"]
    ours = [[chr(c) for c in row[got["cols"]]] for row in got["chars"]] if got["cols"] else [[] for _ in got["chars"]]
    assert ours == ref["columns"]
    assert msgs == ref["warnings"]
    assert got["metadata_columns"] == ref["md_names"]
    assert [[str(v) for v in r] for r in got["metadata_values"]] == [[str(v) for v in r] for r in ref["md_rows"]]


def test_selection_from_files(files):
    got, ref, msgs = _both(files)
    _same(got, ref, msgs)
    assert got["pos_plot"] == [101, 205, 330, 402, 517, 640, 700, 811] and msgs == ["999 not available in the provided fasta file(s)"]
    assert any(c.islower() for row in ref["columns"] for c in row)      # lower-case characters are kept
    for which in (("lrt",), ("sra",), ("srt", "sra"), ("lra", "srt")):
        _same(*_both(files, which=which))
    _same(*_both(files, ntop_links=1))
    _same(*_both(files, ntop_links=2, which=("lrt", "sra")))
    _same(*_both(files, ntop_links=0))
    got, ref, msgs = _both(files, ntop_links=50)                        # larger than the tables
    _same(got, ref, msgs)
    assert "Plot may be cluttered due to large <ntop_links> value" in msgs


def test_selection_links_df_and_range(files):
    df = pd.DataFrame({"pos1": [517, 101, 330], "pos2": [811, 402, 700], "MI": [0.3, 0.2, 0.1]})
    for n in (1, 2, 3, 7):
        got, ref, msgs = _both(files, links_df=df, ntop_links=n)
        _same(got, ref, msgs)
    assert _both(files, links_df=df, ntop_links=1)[0]["pos_plot"] == [517, 811]
    for frm, to in ((100, 210), (330.4, 402.5), (0, 5), (640, 640)):
        _same(*_both(files, from_=frm, to=to))
    assert _both(files, from_=100, to=210)[0]["pos_plot"] == [101, 205, 640, 811]
    for kw, what in ((dict(from_=5), "<to> must"), (dict(to=5), "<from> must"), (dict(from_=9, to=5), "less than"), (dict(from_=-2, to=5), "positive"),
                     (dict(ntop_links=-1), "positive")):
        with pytest.raises(ValueError, match=what):
            _both(files, **kw)


def test_selection_pos_file_edges(files, tmp_path):
    twice = tmp_path / "twice.pos"
    twice.write_text("".join(f"{p}\n" for p in POS[:6] + [205, 811]))      # 205 stands twice, 700 is absent: both dropped with the warning
    got, ref, msgs = _both(files, pos=twice)
    _same(got, ref, msgs)
    assert got["pos_plot"] == [101, 330, 402, 517, 640, 811]
    assert "205 not available in the provided fasta file(s)" in msgs and "700 not available in the provided fasta file(s)" in msgs
    short = tmp_path / "short.pos"
    short.write_text("101\n205\n")
    with pytest.raises(ValueError, match="characters but the position file"):
        T.tree_selection(TIPS, None, files["fasta"], short, None, files["lrt"])


def test_selection_fasta_names(files, tmp_path):
    with pytest.raises(ValueError, match="Sequence names mismatch"):
        _both(files, tips=TIPS + ["iso9"])
    dup = tmp_path / "dup.fa"
    dup.write_text(files["fasta"].read_text() + f">iso1\n{files['seqs'][0]}\n")
    with pytest.raises(ValueError, match="Sequence names mismatch"):
        T.tree_selection(TIPS, None, dup, files["pos"], None, files["lrt"])
    with pytest.raises(ValueError, match="srp column"):
        T.tree_selection(TIPS, None, files["fasta"], files["pos"], None, None, None, files["lrt"])
    with pytest.raises(ValueError, match="must be provided"):
        T.tree_selection(TIPS, None, None, files["pos"])


@pytest.mark.parametrize("idname", ["id", "ID", "Id"])
def test_selection_metadata(files, idname):
    md = pd.DataFrame({"country": ["fi", "se", "no", "fi", "dk", "se", "xx"], idname: ["iso2", "iso0", "iso1", "iso4", "iso3", "iso0", "other"],
                       "year": [2001, 2002, 2003, 2001, 2004, 1999, 2000]})
    got, ref, msgs = _both(files, metadata=md)
    _same(got, ref, msgs)
    assert got["metadata_columns"] == ["country", "year"]
    assert [r[0] for r in got["metadata_values"]] == ["dk", "se", "fi", "no", "fi"]      # a repeated id: the first row
    with pytest.raises(ValueError, match="missing in <metadata_df>"):
        _both(files, metadata=md[md[idname] != "iso4"])
    with pytest.raises(ValueError, match="must contain an ID column"):
        _both(files, metadata=md.rename(columns={idname: "name"}))
    with pytest.raises(ValueError, match="must contain an ID column"):
        _both(files, metadata=md.assign(**{"iD": 1}))


def test_levels_and_palette():
    lev, vals = T.group_levels([[ord("a"), ord("C"), ord("-")], [ord("C"), ord("C"), ord("T")]])
    assert vals == [ord("-"), ord("C"), ord("T"), ord("a")] and lev.tolist() == [[3, 1, 0], [1, 1, 2]]
    lev, vals = T.group_levels([["b", None, "B"]])
    assert vals == ["B", "b"] and lev.tolist() == [[1, 255, 0]]
    from ldweaver_amd.network import hue_palette
    pal = T.group_palette(3)
    assert pal[:3].tolist() == hue_palette(3) and pal[255] == T.MISSING_RGB and pal.shape == (256,)


# ---- the layout ----------------------------------------------------------------------------------------------------------------------------------------------------------

def _meet(a, b):
    return a[0] < b[0] + b[2] and b[0] < a[0] + a[2] and a[1] < b[1] + b[3] and b[1] < a[1] + a[3]


@pytest.mark.parametrize("W,H,nm,na", [(600, 900, 2, 12), (4500, 6000, 3, 40), (300, 400, 0, 5), (300, 400, 2, 0), (200, 200, 0, 0)])
def test_layout_rectangles(W, H, nm, na):
    rng = np.random.default_rng(7)
    tree = T.ladderize(T.midpoint_root(T.parse_newick(random_newick(rng, 37).encode())))
    kw = dict(width_metadata=0.1) if nm else {}
    lay = T.tree_layout(tree, W, H, nm, na, band_labels=["label"] * (nm + na), legends=[("Metadata", ["a", "b"], [1, 2]), ("Alleles", ["A"], [3])], **kw)
    rects = [tuple(lay["panel"])] + [tuple(r) for r in lay["bands"].tolist()]
    assert len(rects) == 1 + nm + na
    for r in rects:
        assert r[0] >= 0 and r[1] >= 0 and r[2] >= 1 and r[3] >= 1 and r[0] + r[2] <= W and r[1] + r[3] <= H
    for i in range(len(rects)):
        for j in range(i):
            assert not _meet(rects[i], rects[j]), (i, j)
    px, py, pw, ph = lay["panel"]
    assert all(r[0] == px and r[2] == pw and r[1] >= py + ph for r in rects[1:])
    bars = lay["bars"]
    assert len(bars) >= tree.n_tips and np.all(bars["x1"] > bars["x0"]) and np.all(bars["y1"] > bars["y0"])
    assert bars["x0"].min() >= 0 and bars["x1"].max() <= 16 * pw and bars["y0"].min() >= 0 and bars["y1"].max() <= 16 * ph
    for (x, y) in lay["legend_xy"]:
        assert x >= px + pw
    # a node lies midway between its first and last child, a tip in the middle of its slot
    order = lay["tip_order"].tolist()
    for slot, t in enumerate(order):
        assert lay["node_x"][tree.tip_node[t]] == int(np.floor((slot + 0.5) * pw / tree.n_tips * 16 + 0.5))


def test_layout_refusals():
    tree = T.parse_newick(b"((A:1,B:1):1,C:3);")
    with pytest.raises(ValueError, match="overlap"):
        T.tree_layout(tree, 600, 900, 2, 12, offset_alleles=0.0, width_metadata=0.5)
    with pytest.raises(ValueError, match="no pixel row"):
        T.tree_layout(tree, 300, 100, 3, 12)
    with pytest.raises(ValueError, match="8192"):
        T.tree_layout(tree, 9000, 100)
    with pytest.raises(ValueError, match="8192"):
        T.view_tree("none.nwk", fasta_path="a", pos_file_path="b", plot_width=30, dpi=300)
