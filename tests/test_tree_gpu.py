"""GPU: the tree view's device renderer (ldw_plot_tree / ldw_debug_plot_tree) against the per-pixel painter of tests/tree_ref.py, bit for bit: bars
at their edges, bands at every ratio of tips to pixels, the limit on the bar count, and view_tree end to end."""
import numpy as np
import pandas as pd
import pytest

import plot_ref as R
import tree_ref as TR
from ldweaver_amd import _lib as L
from ldweaver_amd import tree as T
from ldweaver_amd.engine import Engine

pytestmark = pytest.mark.gpu

PW, PH = 64, 48
CANVAS = (70, 52)
PANEL = (3, 2, PW, PH)
FG = 0x1F4E79


def _bars(rows):
    out = np.zeros(len(rows), dtype=Engine.BAR)
    for k, r in enumerate(rows):
        out[k] = tuple(r)
    return out


def _random_bars(n=2000, seed=3):
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(n):
        x0, y0 = int(rng.integers(-100, 16 * PW + 100)), int(rng.integers(-100, 16 * PH + 100))
        w = int(rng.integers(1, 300)) if k % 3 else int(rng.integers(1, 17))
        h = int(rng.integers(1, 300)) if k % 3 != 1 else int(rng.integers(1, 17))
        rows.append((x0, y0, x0 + w, y0 + h))
    return rows


BAR_CASES = {
    "aligned": [(16, 32, 80, 48)],
    "sixteenth": [(35, 18, 36, 30)],
    "four_pixels": [(40, 40, 56, 56)],
    "outside": [(-40, -8, 24, 8), (16 * PW - 8, 100, 16 * PW + 50, 130), (100, 16 * PH - 3, 130, 16 * PH + 40), (-100, -100, -10, -10), (2000, 10, 2100, 20),
                (-(1 << 20), -(1 << 20), -(1 << 20) + 5, 1 << 20), (16 * PW, 0, 16 * PW + 16, 16), (-16, 0, 0, 16)],
    "cap": [(160, 160, 176, 176)] * 300 + [(320, 320, 328, 328)] * 3 + [(480, 320, 488, 328)] * 5 + [(15, 15, 17, 17)] * 200,
    "wide": [(0, 100, 16 * PW, 116), (-500, 200, 16 * PW + 500, 216), (-(1 << 20), 303, 1 << 20, 310), (500, -(1 << 20), 516, 1 << 20)],
    "random": _random_bars(),
}


@pytest.mark.parametrize("case", list(BAR_CASES))
def test_bars_match_the_painter(engine, case):
    rows = BAR_CASES[case]
    got = engine.plot_tree_raster(*CANVAS, PANEL, _bars(rows), FG)
    want = TR.paint_canvas(*CANVAS, PANEL, rows, FG, [], [], [])
    assert got.shape == want.shape and np.array_equal(got, want), np.argwhere(np.any(got != want, axis=2))[:5]
    if case == "cap":
        x, y = PANEL[0] + 10, PANEL[1] + 10
        assert tuple(got[y, x]) == ((FG >> 16) & 255, (FG >> 8) & 255, FG & 255)
    if case != "outside":
        assert np.any(got != 255)
    assert np.all(got[:PANEL[1]] == 255) and np.all(got[:, :PANEL[0]] == 255) and np.all(got[PANEL[1] + PH:] == 255) and np.all(got[:, PANEL[0] + PW:] == 255)


def _caterpillar(n):
    return ("(" * (n - 1) + "t0:1" + "".join(f",t{k}:1):1" for k in range(1, n)))[:-2] + ";"


@pytest.mark.parametrize("kind", ["caterpillar", "star"])
def test_laid_out_trees_match_the_painter(engine, kind):
    n = 500
    text = _caterpillar(n) if kind == "caterpillar" else "(" + ",".join(f"t{k}:{1 + k % 7}" for k in range(n)) + ");"
    tree = T.ladderize(T.parse_newick(text.encode()))
    lay = T.tree_layout(tree, 76, 70)
    assert lay["panel"][2] <= PW and lay["panel"][3] <= PH and len(lay["bars"]) >= n
    rows = [tuple(int(v) for v in b) for b in lay["bars"].tolist()]
    got = engine.plot_tree_raster(76, 70, lay["panel"], lay["bars"], 0)
    want = TR.paint_canvas(76, 70, lay["panel"], rows, 0, [], [], [])
    assert np.array_equal(got, want), np.argwhere(np.any(got != want, axis=2))[:5]
    assert np.any(got != 255)


BW = 16


@pytest.mark.parametrize("bands", [1, 2, 7])
@pytest.mark.parametrize("N,W", [(2, BW), (BW - 1, BW), (BW, BW), (BW + 1, BW), (3 * BW + 1, BW), (40 * BW, BW), (5, 1), (1, BW)])
def test_bands_match_the_painter(engine, N, W, bands):
    rng = np.random.default_rng(100 * N + bands)
    lev = rng.integers(0, 6, (bands, N)).astype(np.uint8)
    lev[rng.random((bands, N)) < 0.15] = 255
    lev[0, N - 1] = 255
    pal = rng.integers(0, 1 << 24, (bands, 256)).astype(np.uint32)
    pal[:, 255] = T.MISSING_RGB
    heights = [1 + (r % 3) for r in range(bands)]
    rects, y = [], 5
    for r in range(bands):
        rects.append((2, y, W, heights[r]))
        y += heights[r] + (r % 2)
    cw, ch = 20, y + 1
    panel = (0, 0, cw, 4)
    bars = [(8, 8, 24, 40)]
    got = engine.plot_tree_raster(cw, ch, panel, _bars(bars), FG, lev, pal, rects)
    want = TR.paint_canvas(cw, ch, panel, bars, FG, lev, pal, rects)
    assert np.array_equal(got, want), np.argwhere(np.any(got != want, axis=2))[:5]
    if N <= 3 * BW + 1:      # the painter's restricted loop over tips equals the loop over all of them
        for r in range(bands):
            assert np.array_equal(TR.paint_band_line(lev[r], pal[r], W), TR.paint_band_line_fast(lev[r], pal[r], W))


def test_refusals(engine):
    too_many = np.zeros((1 << 23) + 1, dtype=Engine.BAR)      # (empty bars too: the count is looked at first)
    with pytest.raises(L.LdwError, match=r"8388609 bars") as e:
        engine.plot_tree_raster(*CANVAS, PANEL, too_many, FG)
    assert e.value.code == L.LDW_ERR_ARG
    for bad, what in (([(0, 0, 0, 16)], "empty"), ([(0, 0, (1 << 20) + 1, 16)], "coordinate"), ([(5, 9, 4, 16)], "empty")):
        with pytest.raises(L.LdwError, match=what):
            engine.plot_tree_raster(*CANVAS, PANEL, _bars(bad), FG)
    with pytest.raises(L.LdwError, match="leaves the canvas"):
        engine.plot_tree_raster(*CANVAS, (10, 10, PW, PH), _bars([]), FG)
    lev, pal = np.zeros((2, 4), dtype=np.uint8), np.zeros((2, 256), dtype=np.uint32)
    with pytest.raises(L.LdwError, match="overlaps the panel"):
        engine.plot_tree_raster(*CANVAS, (0, 0, 20, 20), _bars([]), FG, lev, pal, [(30, 30, 5, 5), (19, 19, 5, 5)])
    with pytest.raises(L.LdwError, match="bands 0 and 1 overlap"):
        engine.plot_tree_raster(*CANVAS, (0, 0, 20, 20), _bars([]), FG, lev, pal, [(30, 30, 5, 5), (34, 34, 5, 5)])
    blank = engine.plot_tree_raster(*CANVAS, PANEL, _bars([]), FG)      # no bars, no bands: a white canvas; the context works on
    assert np.all(blank == 255)


def _random_tree(rng, n):
    items = [f"s{k}:{round(float(rng.random()) + 0.05, 3)}" for k in range(n)]
    while len(items) > 1:
        k = min(len(items), int(rng.integers(2, 4)))
        pick = sorted(rng.choice(len(items), k, replace=False).tolist(), reverse=True)
        grp = [items.pop(j) for j in pick]
        items.append("(" + ",".join(grp) + ")" + (f":{round(float(rng.random()) + 0.05, 3)}" if items else ""))
    return items[0] + ";"


def test_view_tree_end_to_end(engine, tmp_path):
    rng = np.random.default_rng(42)
    n, npos = 40, 12
    (tmp_path / "t.nwk").write_text(_random_tree(rng, n))
    pos = sorted(rng.choice(np.arange(100, 5000), npos, replace=False).tolist())
    (tmp_path / "s.pos").write_text("".join(f"{p}\n" for p in pos))
    (tmp_path / "s.fa").write_text("".join(f">s{k}\n{''.join(rng.choice(list('ACGTNa'), npos))}\n" for k in rng.permutation(n)))
    rows = [(pos[2 * k], pos[2 * k + 1], pos[2 * k + 1] - pos[2 * k], round(0.9 - 0.1 * k, 2), 1, "nsXns") for k in range(6)]
    (tmp_path / "lr_tophits.tsv").write_text("pos1\tpos2\tlen\tMI\tARACNE\tlinks\n" + "".join("\t".join(str(v) for v in r) + "\n" for r in rows))
    md = pd.DataFrame({"id": [f"s{k}" for k in range(n)], "country": [["fi", "se", None, "no"][k % 4] for k in range(n)], "yr": [2000 + k % 3 for k in range(n)]})
    kw = dict(metadata_df=md, fasta_path=tmp_path / "s.fa", pos_file_path=tmp_path / "s.pos", lr_tophits_path=tmp_path / "lr_tophits.tsv", width_metadata=0.2,
              offset_alleles=0.3, width_alleles=1.5, plot_height=5, plot_width=5, dpi=30, engine=engine)
    png = tmp_path / "tree.png"
    out = T.view_tree(tmp_path / "t.nwk", plot_save_path=png, want_canvas=True, **kw)
    lay, canvas = out["layout"], out["canvas"]
    W, H = lay["canvas"]
    assert (W, H) == (150, 150) and canvas.shape == (H, W, 3)
    assert out["pos_plot"] == pos and out["metadata_columns"] == ["country", "yr"] and len(lay["bands"]) == 14
    px, py, pw, ph = lay["panel"]
    assert pw <= PW and ph <= PH
    assert np.any(out["levels"][0] == 255) and sorted(out["metadata"][1]) == ["2000", "2001", "2002", "fi", "no", "se"]
    rows = [tuple(int(v) for v in b) for b in lay["bars"].tolist()]
    want = TR.paint_canvas(W, H, lay["panel"], rows, T.TREE_RGB, out["levels"], out["palette"], lay["bands"])
    covered = np.zeros((H, W), dtype=bool)
    for x, y, w, h in [lay["panel"]] + lay["bands"].tolist():
        assert np.array_equal(canvas[y:y + h, x:x + w], want[y:y + h, x:x + w])
        covered[y:y + h, x:x + w] = True
    assert np.any(canvas[py:py + ph, px:px + pw] != 255)
    boxes = out["boxes"]
    assert boxes.shape == (14 + 3, 4) and np.all(boxes[:, 2] > 0)
    drawn = np.zeros((H, W), dtype=bool)
    for x, y, w, h in boxes.tolist():
        assert not np.any(covered[max(y, 0):y + h, max(x, 0):x + w]), "the host drew over the panel or a band"
        assert np.any(canvas[max(y, 0):y + h, max(x, 0):x + w] != 255)
        drawn[max(y, 0):y + h, max(x, 0):x + w] = True
    assert np.all(canvas[~covered & ~drawn] == 255)
    raster = engine.plot_tree_raster(W, H, lay["panel"], lay["bars"], T.TREE_RGB, out["levels"], out["palette"], lay["bands"])
    assert np.array_equal(raster, want) and np.array_equal(raster[~drawn], canvas[~drawn])
    decoded, _ = R.png_decode(png.read_bytes())
    assert np.array_equal(decoded, canvas)
    again = T.view_tree(tmp_path / "t.nwk", plot_save_path=None, **kw)
    assert again["png"] is None and np.array_equal(again["canvas"], canvas) and np.array_equal(again["boxes"], boxes)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["lr_tophits.tsv", "s.fa", "s.pos", "t.nwk", "tree.png"]
