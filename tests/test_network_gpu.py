"""GPU: the device search of annotated link files (ldw_links_grep) against pandas + str.contains(regex=False) + the two filters, its refusals,
create_network_for_gene's native route against its pandas route, the capsule renderer against the naive painter of tests/network_ref.py, and
the PNG of create_network end to end."""
import ctypes as C
import gzip
import os

import numpy as np
import pandas as pd
import pytest

import network_ref as NR
import plot_ref as R
from ldweaver_amd import _lib as L
from ldweaver_amd import annotate as A
from ldweaver_amd import network as N
from test_network_host import LR_COLS, SR_COLS, gene_files

pytestmark = pytest.mark.gpu

LONG = ("L" + "0123456789" * 26)[:255]          # a 255-byte needle
assert len(LONG) == 255


def _rows(n=300, seed=11):
    rng = np.random.default_rng(seed)
    genes = ["pbp2x", "pbp2xL", "pbp1a", "dnaA", "DnaA", "gyrB", "parC", "folA"]
    links = ["syXsy", "nsXsy", "syXns", "nsXns", "syXsyX"]
    rows = []
    for k in range(n):
        a, b = rng.choice(len(genes), 2)
        p1 = int(rng.integers(1, 2_000_000))
        rows.append(dict(pos1=p1, pos2=p1 + int(rng.integers(1, 90000)), len=int(rng.integers(1, 90000)), ARACNE=int(rng.random() < 0.6), MI=repr(round(float(rng.random()), 9)),
                         srp=repr(round(float(rng.random() * 7), 5)), pos1_ann=f"{genes[a]}:{rng.integers(1, 999)}:missense_variant", pos2_ann=f"{genes[b]}:{rng.integers(1, 999)}:syn",
                         pos1_genreg=f"{genes[a]}_reg", pos2_genreg="ONLYGENREG" if k % 7 == 0 else "reg", links=str(rng.choice(links)), pos1_ad="A:0.41", pos2_ad="G:0.07"))
    # the crafted rows
    rows[5].update(pos1_ann="abcX:1", pos2_ann="Yabc")                    # a needle at the first byte of one field and at the last of the other
    rows[17].update(pos1_ann="wholefield", pos2_ann="zz")                 # a needle equal to the whole field
    rows[29].update(pos1_ann="short", pos2_ann="q")                       # ... and one longer than the field
    rows[40].update(pos1_ann="xx_end", pos2_ann="beg_yy")                 # "end\tbeg" exists only across the tab
    rows[52].update(pos1_ann="", pos2_ann="afterempty:3")                 # an empty pos1_ann
    rows[53].update(pos1_ann="", pos2_ann="")
    rows[66].update(pos1_ann="k:1", pos2_ann="pre" + LONG + "post")
    rows[80].update(pos1_ann="needle64here", pos2_ann="n")
    rows[81].update(links="syXsyX", ARACNE=1, pos1_ann="abc")
    rows[82].update(links="syXsy", ARACNE=1, pos1_ann="abc")
    rows[83].update(links="nsXns", ARACNE=0, pos1_ann="abc")
    rows[84].update(links="nsXns", ARACNE="1e+00", pos1_ann="abc")
    rows[85].update(links="nsXns", ARACNE="0", pos1_ann="abc")
    rows[86].update(links="nsXns", ARACNE="1.00000000000000000000000", pos1_ann="abc", MI="0.1234567890123456789012")      # slow cells: the host's strtod
    rows[n - 1].update(pos1_ann="lastrow:abc")
    return rows


def _write(path, cols, rows, eol="\n", last_newline=True, blank_after=None):
    lines = ["\t".join(cols)] + ["\t".join(str(r[c]) for c in cols) for r in rows]
    if blank_after is not None:
        lines.insert(blank_after, "")
    text = eol.join(lines) + (eol if last_newline else "")
    data = text.encode()
    if str(path).endswith(".gz"):
        with gzip.open(path, "wb") as fh:
            fh.write(data)
    else:
        with open(path, "wb") as fh:
            fh.write(data)
    return str(path)


NEEDLE_SETS = {
    "one": ["abc"],
    "edges": ["abc", "wholefield", "shorter", "end\tbeg", "endbeg", "ONLYGENREG", "afterempty", "pbp2x", "pbp2xL", "dnaA", "DnaA", LONG, LONG[:-1] + "x", "absent"],
    "n64": [f"absent{k}" for k in range(63)] + ["needle64here"],
    "n65": [f"absent{k}" for k in range(64)] + ["needle64here"],           # only needle 64 (the second mask word) matches
    "none": ["nothing_matches_this"],
}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("grep")
    rows = _rows()
    perm = [SR_COLS[i] for i in (7, 3, 12, 0, 10, 5, 1, 6, 9, 2, 11, 4, 8)]
    out = {
        "sr": _write(d / "sr.tsv", SR_COLS, rows),
        "lr": _write(d / "lr.tsv", LR_COLS, rows),
        "gz": _write(d / "sr.tsv.gz", SR_COLS, rows),
        "crlf": _write(d / "crlf.tsv", SR_COLS, rows, eol="\r\n"),
        "nonl": _write(d / "nonl.tsv", SR_COLS, rows, last_newline=False),
        "blank": _write(d / "blank.tsv", SR_COLS, rows, blank_after=150),
        "perm": _write(d / "perm.tsv", perm, rows),
        "header_only": _write(d / "header_only.tsv", SR_COLS, []),
    }
    return out, {k: NR.read_annotated(p) for k, p in out.items()}


def _expect(tab, needles, drop_sy, drop_ind):
    nw = (len(needles) + 63) // 64
    mask = np.zeros((len(tab), nw), dtype=np.uint64)
    for j, nd in enumerate(needles):
        hit = (tab["pos1_ann"].str.contains(nd, regex=False) | tab["pos2_ann"].str.contains(nd, regex=False)).to_numpy(dtype=bool)
        mask[hit, j >> 6] |= np.uint64(1) << np.uint64(j & 63)
    keep = mask.any(axis=1)
    if drop_sy:
        keep &= (tab["links"] != "syXsy").to_numpy()
    if drop_ind:
        keep &= (tab["ARACNE"].to_numpy(dtype=float) == 1)
    idx = np.nonzero(keep)[0]
    return idx, mask[idx]


def _check(engine, path, tab, needles, drop_sy, drop_ind, chunk):
    got = engine.links_grep(path, needles, drop_sy, drop_ind, chunk)
    idx, mask = _expect(tab, needles, drop_sy, drop_ind)
    assert got["data_rows"] == len(tab)
    assert np.array_equal(got["row"], idx), (path, needles[:3], drop_sy, drop_ind)
    for k, c in enumerate(("pos1", "pos2", "len", "ARACNE", "MI")):
        assert np.array_equal(got["num"][:, k], tab[c].to_numpy(dtype=float)[idx]), c
    for c in ("pos1_ann", "pos2_ann", "links"):
        assert [b.decode() for b in got[c]] == tab[c].iloc[idx].tolist(), c
    assert np.array_equal(got["mask"], mask)
    return len(idx)


@pytest.mark.parametrize("kind", ["sr", "lr", "gz", "crlf", "nonl", "blank", "perm"])
def test_search_matches_pandas(engine, files, kind):
    paths, tabs = files
    for chunk in (0, 4096):           # 4 KiB: rows and string fields straddle the chunk cuts
        for name, needles in NEEDLE_SETS.items():
            n = _check(engine, paths[kind], tabs[kind], needles, False, False, chunk)
            assert (n == 0) == (name == "none")
    for ds in (False, True):
        for di in (False, True):
            _check(engine, paths[kind], tabs[kind], NEEDLE_SETS["edges"], ds, di, 4096)


def test_search_edge_semantics(engine, files):
    """What the comparisons above rest on, stated directly."""
    paths, tabs = files
    t = tabs["sr"]
    g = engine.links_grep(paths["sr"], NEEDLE_SETS["edges"])
    by_row = {int(r): int(m) for r, m in zip(g["row"], g["mask"][:, 0])}
    nd = NEEDLE_SETS["edges"]
    bit = lambda s: 1 << nd.index(s)
    assert by_row[5] & bit("abc") and by_row[17] & bit("wholefield") and 29 not in by_row
    assert 40 not in by_row                                                         # nothing matches across the tab
    assert not any(m & (bit("ONLYGENREG") | bit("end\tbeg") | bit("endbeg") | bit("shorter") | bit("absent")) for m in by_row.values())
    assert by_row[52] == bit("afterempty") and 53 not in by_row
    assert by_row[66] == bit(LONG)                                                  # the 255-byte needle, not its neighbour with another last byte
    assert by_row[299] & bit("abc")
    both = [m for m in by_row.values() if m & bit("pbp2xL")]
    assert both and all(m & bit("pbp2x") for m in both) and any(m & bit("pbp2x") and not m & bit("pbp2xL") for m in by_row.values())
    assert any(m & bit("dnaA") and not m & bit("DnaA") for m in by_row.values()) and any(m & bit("DnaA") and not m & bit("dnaA") for m in by_row.values())
    g = engine.links_grep(paths["sr"], NEEDLE_SETS["n65"])
    assert g["row"].tolist() == [80] and g["mask"].tolist() == [[0, 1]]
    g = engine.links_grep(paths["sr"], NEEDLE_SETS["n64"])
    assert g["row"].tolist() == [80] and g["mask"].tolist() == [[1 << 63]]
    # the filters on rows 81..86: syXsyX stays; ARACNE 1, 1e+00 and the slow 1.000...0 are 1
    g = engine.links_grep(paths["sr"], ["abc"], True, True)
    kept = set(g["row"].tolist())
    assert {81, 84, 86} <= kept and not {82, 83, 85} & kept
    assert g["num"][g["row"].tolist().index(86), 4] == float("0.1234567890123456789012")
    g = engine.links_grep(paths["sr"], ["abc"], True, False)
    assert {81, 83, 84, 85, 86} <= set(g["row"].tolist()) and 82 not in g["row"]
    g = engine.links_grep(paths["header_only"], ["abc"])
    assert len(g["row"]) == 0 and g["data_rows"] == 0 and g["mask"].shape == (0, 1)
    g = engine.links_grep(paths["sr"], [b"abc"] * 1024)
    assert g["mask"].shape[1] == 16 and (g["mask"] == np.uint64(2 ** 64 - 1)).all()


def test_search_of_a_file_the_library_wrote(engine, tmp_path):
    """annotate.write_links_table's own output (the long-range file holds ARACNE as TRUE / FALSE)."""
    n = 300
    rng = np.random.default_rng(2)
    table = [f"g{k}:{k}:x" for k in range(20)] + ["syXsy", "nsXns"] + ["FALSE", "TRUE"]
    r1, r2 = rng.integers(0, 20, n).astype(np.int32), rng.integers(0, 20, n).astype(np.int32)
    pair, ar = rng.integers(0, 2, n).astype(np.int32), rng.integers(0, 2, n).astype(np.int32)
    num = [("pos1", L.COL_INT64, np.arange(n, dtype=np.int64) + 1), ("pos2", L.COL_INT64, np.arange(n, dtype=np.int64) + 70), ("len", L.COL_DOUBLE, np.full(n, 69.0)),
           ("MI", L.COL_DOUBLE, rng.random(n))]
    strs = [("pos1_ann", 0, r1), ("pos2_ann", 0, r2), ("pos1_genreg", 0, r1), ("pos2_genreg", 0, r2), ("pos1_ad", 0, r1), ("pos2_ad", 0, r2), ("links", 20, pair),
            ("ARACNE", 22, ar)]
    path = str(tmp_path / "lr_links_annotated.tsv")
    A.write_links_table(path, A.LR_COLS, num, strs, table)
    g = engine.links_grep(path, ["g7:", "g19:19"], True, True, 4096)
    want = [i for i in range(n) if (r1[i] in (7, 19) or r2[i] in (7, 19)) and pair[i] == 1 and ar[i] == 1]
    assert g["row"].tolist() == want and len(want) > 3 and (g["num"][:, 3] == 1).all()
    assert [b.decode() for b in g["pos1_ann"]] == [table[r1[i]] for i in want]


def test_search_keeps_more_rows_than_the_first_record_buffer(engine, tmp_path):
    """A chunk gets room for 16384 kept rows at first; one that keeps more is searched again with room for all of them (include/ldweaver_amd.h 14)."""
    n = 20000
    cols = ("pos1_ann", "MI", "pos2_ann", "links", "ARACNE", "len", "pos2", "pos1")
    path = tmp_path / "many.tsv"
    path.write_text("\t".join(cols) + "\n" + "".join(f"g{k % 7}\t0.5\th\tnsXns\t{k % 2}\t3\t{k + 3}\t{k}\n" for k in range(n)))
    g = engine.links_grep(str(path), ["g", "g3"])
    assert np.array_equal(g["row"], np.arange(n)) and np.array_equal(g["num"][:, 0], np.arange(n, dtype=float))
    assert np.array_equal(g["mask"][:, 0], np.where(np.arange(n) % 7 == 3, 3, 1).astype(np.uint64))
    assert [b.decode() for b in g["pos1_ann"][:8]] == [f"g{k % 7}" for k in range(8)] and g["data_rows"] == n
    g = engine.links_grep(str(path), ["g"], False, True)
    assert np.array_equal(g["row"], np.arange(1, n, 2))          # 10000 kept: the first buffer holds them
    g = engine.links_grep(str(path), ["g"], False, False, 65536)  # several chunks, each below the first buffer
    assert np.array_equal(g["row"], np.arange(n))


def test_search_refusals(engine, files, tmp_path):
    paths, _ = files
    rows = _rows(120)

    def refused(path, *words, needles=("abc",), chunk=4096):
        with pytest.raises(L.LdwError) as e:
            engine.links_grep(path, list(needles), False, False, chunk)
        msg = str(e.value)
        for w in (os.path.basename(path),) + words:
            assert w in msg, (w, msg)
        return msg

    cols = [c for c in SR_COLS if c != "pos2_ann"]
    refused(_write(tmp_path / "nohdr.tsv", cols, rows), "line 1, column 13", '"pos2_ann"')
    cols = list(SR_COLS)
    cols[8] = "MI"
    refused(_write(tmp_path / "twice.tsv", cols, [dict(r, MI=r["MI"]) for r in rows]), "line 1, column 9", '"MI"')

    def lines_of(rows):
        return ["\t".join(SR_COLS)] + ["\t".join(str(r[c]) for c in SR_COLS) for r in rows]

    def put(name, lines):
        p = tmp_path / name
        p.write_text("\n".join(lines) + "\n")
        return str(p)

    ln = lines_of(rows)
    short = list(ln)
    short[60] = short[60].rsplit("\t", 1)[0]
    refused(put("short.tsv", short), "line 61, column 13")
    long_ = list(ln)
    long_[61] += "\textra"
    refused(put("long.tsv", long_), "line 62, column 14")
    bad = [dict(r) for r in rows]
    bad[99]["MI"] = "abc"
    refused(put("abc.tsv", lines_of(bad)), "line 101, column 5", "not a number")
    two = list(long_)
    two[20] = two[20].rsplit("\t", 1)[0]           # an earlier bad line, in an earlier chunk
    refused(put("two.tsv", two), "line 21, column 13")
    two[10] = ""                                   # an empty line in front: physical lines count
    refused(put("two_b.tsv", two), "line 21, column 13")
    assert L.lib().ldw_links_grep_fetch(engine._ctx, 0, 0, None, None, None, None, None) == L.LDW_ERR_STATE     # no result after a refusal
    # needles out of range
    for nd in ([], ["x"] * 1025, [""], ["y" * 256]):
        with pytest.raises(L.LdwError):
            engine.links_grep(paths["sr"], nd)
    with pytest.raises(FileNotFoundError):
        engine.links_grep(str(tmp_path / "nothing.tsv"), ["a"])
    assert len(engine.links_grep(paths["sr"], ["abc"])["row"]) > 0      # the engine works on


def test_host_trim_releases_the_search_buffers(engine, files):
    paths, tabs = files
    engine.links_grep(paths["sr"], ["abc"])
    n = C.c_int64(0)
    L.check(L.lib().ldw_host_trim(engine._ctx, C.byref(n)))
    assert n.value > 0
    assert L.lib().ldw_links_grep_fetch(engine._ctx, 0, 0, None, None, None, None, None) == L.LDW_ERR_STATE
    _check(engine, paths["sr"], tabs["sr"], ["abc"], False, False, 0)


@pytest.mark.parametrize("level", [1, 2])
def test_for_gene_native_equals_pandas(engine, tmp_path, level):
    sr, lr = gene_files(tmp_path)
    seen = 0
    for gene in ("pbp2x", "pbp1a", "pbp", "absent"):
        for kw in (dict(), dict(drop_syXsy=False, drop_indirect=False, min_links_to_include=1)):
            a = N.create_network_for_gene(gene, sr, lr, level=level, engine=engine, reader="native", chunk_bytes=4096, **kw)
            b = N.create_network_for_gene(gene, sr, lr, level=level, reader="pandas", **kw)
            assert list(a.columns) == NR.FRAME_COLS and len(a) == len(b)
            if len(b):
                pd.testing.assert_frame_equal(a, b, check_exact=True)
            seen += len(b)
    only_lr = N.create_network_for_gene("dnaA", None, lr, level=level, engine=engine)
    pd.testing.assert_frame_equal(only_lr, N.create_network_for_gene("dnaA", None, lr, level=level, reader="pandas"), check_exact=True)
    assert seen > 100


# ---- the renderer ---------------------------------------------------------------------------------------------------------------------------

W, H = 96, 70      # no multiple of the 32-pixel tile


def _same(engine, caps):
    got = engine.plot_capsules(np.array(caps, dtype=engine.CAPSULE), W, H)
    want = NR.paint(caps, W, H)
    assert got.shape == (H, W, 3) and np.array_equal(got, want)
    return got


def test_raster_discs_and_segments(engine):
    img = _same(engine, [(10, 10, 10, 10, 1, 0x000000, 255), (30, 10, 30, 10, 2, 0x000000, 255), (50, 12, 50, 12, 9, 0x102030, 255)])
    assert (img[10, 10] == 0).all() and (img[10, 11] == 255).all()                    # width 1: the pixel itself
    assert (img[10, 31] == 0).all() and (img[11, 31] == 255).all()                    # width 2: the four neighbours too
    _same(engine, [(3, 20, 92, 20, 3, 0xFF0000, 200), (40, 2, 40, 68, 4, 0x00FF00, 128), (5, 5, 90, 66, 5, 0x0000FF, 90), (90, 3, 8, 60, 2, 0x123456, 255),
                   (31, 31, 32, 32, 1, 0x000000, 255), (63, 0, 64, 69, 7, 0x808080, 17)])
    _same(engine, [(-50, -50, -20, -30, 6, 0xFF00FF, 255), (200, 10, 300, 40, 9, 0x00FFFF, 255), (-30, 35, 50, 35, 8, 0xFFAA00, 160), (80, 60, 140, 120, 11, 0x0055AA, 77),
                   (-8192, -8192, 16383, 16383, 1024, 0x010203, 1)])
    assert (_same(engine, []) == 255).all()


def test_raster_blends_in_list_order(engine):
    a, b = (10, 30, 80, 40, 12, 0xFF0000, 140), (20, 50, 70, 20, 14, 0x0000FF, 90)
    ab, ba = _same(engine, [a, b]), _same(engine, [b, a])
    assert not np.array_equal(ab, ba)


def test_raster_many_capsules_through_one_tile(engine):
    rng = np.random.default_rng(4)
    caps = [(int(rng.integers(28, 68)), int(rng.integers(28, 68)), int(rng.integers(28, 68)), int(rng.integers(28, 68)), int(rng.integers(1, 6)),
             int(rng.integers(0, 1 << 24)), int(rng.integers(1, 256))) for _ in range(300)]
    _same(engine, caps)


def test_raster_refusals(engine):
    for bad in [(0, 0, 0, 20000, 1, 0, 255), (0, 0, 1, 1, 0, 0, 255), (0, 0, 1, 1, 1, 0, 0), (0, 0, 1, 1, 1, 0, 256), (0, -9000, 1, 1, 1, 0, 9), (0, 0, 1, 1, 1025, 0, 9)]:
        with pytest.raises(L.LdwError):
            engine.plot_capsules(np.array([bad], dtype=engine.CAPSULE), W, H)
    with pytest.raises(L.LdwError):
        engine.plot_capsules(np.array([], dtype=engine.CAPSULE), 9000, 10)


def test_create_network_png(engine, tmp_path):
    sr, lr = gene_files(tmp_path)
    hits = N.create_network_for_gene("pbp2x", sr, lr, level=2, engine=engine, drop_syXsy=False, drop_indirect=False, min_links_to_include=1)
    path = tmp_path / "net.png"
    r = N.create_network(hits, netplot_path=str(path), plot_title="pbp2x", plot_w=600, plot_h=400, engine=engine)
    pd.testing.assert_frame_equal(r["edges"], NR.edges(hits), check_exact=True)
    dec, ihdr = R.png_decode(path.read_bytes())
    assert dec.shape == (400, 600, 3) and ihdr[:2] == (600, 400) and r["png"] == str(path)
    raster = engine.plot_capsules(r["capsules"], 600, 400)
    drawn = np.zeros((400, 600), dtype=bool)
    boxes = r["boxes"]
    assert boxes.shape == (len(r["nodes"]) + 2, 4) and boxes[-1, 2] > 0 and boxes[-2, 2] > 0
    for x, y, w, h in boxes.tolist():
        drawn[max(y, 0):max(y + h, 0), max(x, 0):max(x + w, 0)] = True
    assert np.array_equal(dec[~drawn], raster[~drawn]) and (~drawn).sum() > 100000
    assert not np.array_equal(dec[drawn], raster[drawn])            # the labels are there
    assert (raster != 255).any()
