"""GPU: the tanglegram's rectangle pass over the capsule raster (ldw_debug_plot_marks) against the naive painter of tests/tanglegram_ref.py, its
refusals, and the PNGs of create_tanglegram end to end."""
import ctypes as C
import os

import numpy as np
import pytest

import plot_ref as R
import tanglegram_ref as TR
from ldweaver_amd import _lib as L
from ldweaver_amd import tanglegram as T
from test_tanglegram_host import genome, make_tophits, record

pytestmark = pytest.mark.gpu

W, H = 97, 70      # no multiple of the 32-pixel tile

CAPS = [(3, 20, 92, 20, 3, 0xFF0000, 200), (40, 2, 40, 68, 4, 0x00FF00, 128), (5, 5, 90, 66, 5, 0x0000FF, 90), (90, 3, 8, 60, 2, 0x123456, 255),
        (31, 31, 33, 33, 2, 0x000000, 255), (63, 0, 64, 69, 7, 0x808080, 17), (-30, 35, 50, 35, 8, 0xFFAA00, 160), (80, 60, 140, 120, 11, 0x0055AA, 77),
        (22, 14, 26, 16, 2, 0x00AAFF, 255), (24, 12, 24, 18, 1, 0xAA00FF, 99),          # wholly under the two overlapping rectangles
        (96, 69, 96, 69, 1, 0x112233, 255), (70, 40, 75, 44, 3, 0x336699, 200)]         # under the 1 x 1 rectangle; under nothing
RECTS = [(15, 8, 40, 22, 0x4682B4), (28, 10, 60, 30, 0xBEBEBE),        # overlapping, different colours: the later one wins
         (-10, -7, 12, 9, 0x010203), (90, 60, 120, 90, 0x040506),        # past the left and top edges, negative corner; past the right and bottom edges
         (50, 50, 50, 60, 0xFF00FF), (45, 55, 60, 55, 0xFF00FF),         # empty: x0 = x1, y0 = y1
         (W - 1, H - 1, W, H, 0xABCDEF),                                 # 1 x 1 in the last corner
         (31, 40, 34, 42, 0x00FF7F), (20, 31, 25, 34, 0x7F00FF)]         # across the tile edges x = 31..33 and y = 31..33
EVERYWHERE = (-5, -9, 130, 99, 0x202020)                                # past every canvas edge


def _same(engine, caps, rects):
    got = engine.debug_plot_marks(np.array(caps, dtype=engine.CAPSULE), np.array(rects, dtype=engine.RECT), W, H)
    want = TR.paint_marks(caps, rects, W, H)
    assert got.shape == (H, W, 3) and got.dtype == np.uint8 and np.array_equal(got, want)
    return got


def test_rectangles_over_capsules(engine):
    img = _same(engine, CAPS, RECTS)
    assert img[15, 30].tolist() == [0xBE, 0xBE, 0xBE] and img[15, 20].tolist() == [0x46, 0x82, 0xB4]      # the later rectangle where both lie
    assert img[0, 0].tolist() == [1, 2, 3] and img[H - 1, W - 1].tolist() == [0xAB, 0xCD, 0xEF] and img[H - 1, W - 2].tolist() == [4, 5, 6]
    assert img[41, 33].tolist() == [0, 0xFF, 0x7F] and img[41, 34].tolist() != [0, 0xFF, 0x7F]            # half-open across the tile edge
    caps_only = engine.plot_capsules(np.array(CAPS, dtype=engine.CAPSULE), W, H)
    free = np.ones((H, W), dtype=bool)
    for x0, y0, x1, y1, _ in RECTS:
        free[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = False
    assert np.array_equal(img[free], caps_only[free]) and (caps_only[free] != 255).any() and (caps_only[~free] != 255).any()
    assert not np.array_equal(_same(engine, CAPS, RECTS[:2][::-1] + RECTS[2:]), img)                       # list order decides


def test_a_rectangle_past_every_edge(engine):
    under = _same(engine, CAPS, [EVERYWHERE] + RECTS)                  # the others still lie over it
    assert under[45, 72].tolist() == [0x20] * 3 and under[15, 30].tolist() == [0xBE] * 3
    over = _same(engine, CAPS, RECTS + [EVERYWHERE])                   # last in the list: it hides every capsule and every rectangle
    assert (over == 0x20).all()


def test_no_rectangles_is_the_capsule_raster(engine):
    caps = np.array(CAPS, dtype=engine.CAPSULE)
    none = np.zeros(0, dtype=engine.RECT)
    assert engine.debug_plot_marks(caps, none, W, H).tobytes() == engine.plot_capsules(caps, W, H).tobytes()
    only_empty = np.array([RECTS[4], RECTS[5]], dtype=engine.RECT)
    assert engine.debug_plot_marks(caps, only_empty, W, H).tobytes() == engine.plot_capsules(caps, W, H).tobytes()
    assert (engine.debug_plot_marks(np.zeros(0, dtype=engine.CAPSULE), none, W, H) == 255).all()
    img, ms = engine.debug_plot_marks(caps, np.array(RECTS, dtype=engine.RECT), W, H, timings=True)
    assert len(ms) == 3 and all(t >= 0 for t in ms) and np.array_equal(img, TR.paint_marks(CAPS, RECTS, W, H))


def test_many_rectangles_more_than_one_block(engine):
    # 3000 small rectangles (a dozen blocks of the pixel list) and two that span rows wider than a wave: every pixel's owner is the last that covers it
    rng = np.random.default_rng(8)
    rects = [(0, 10, W, 14, 0x111111), (3, 0, 90, H, 0x222222)]
    for _ in range(3000):
        x, y = int(rng.integers(-4, W)), int(rng.integers(-4, H))
        rects.append((x, y, x + int(rng.integers(0, 6)), y + int(rng.integers(0, 6)), int(rng.integers(0, 1 << 24))))
    _same(engine, CAPS[:3], rects)


def test_refusals(engine):
    caps = np.array(CAPS[:2], dtype=engine.CAPSULE)

    def refused(rects, caps=caps, w=W, h=H, match=None):
        with pytest.raises(L.LdwError) as e:
            engine.debug_plot_marks(caps, np.array(rects, dtype=engine.RECT), w, h)
        assert e.value.code == L.LDW_ERR_ARG and (match is None or match in str(e.value)), str(e.value)

    refused([(0, 0, 1, 1, 0)] * ((1 << 16) + 1), match="65537 rectangles")
    engine.debug_plot_marks(caps, np.array([(0, 0, 1, 1, 0)] * (1 << 16), dtype=engine.RECT), W, H)
    for bad in [(-8193, 0, 1, 1, 0), (0, -8193, 1, 1, 0), (0, 0, 16384, 1, 0), (0, 0, 1, 16384, 0)]:
        refused([RECTS[0], bad], match="rectangle 1 has a coordinate outside")
    engine.debug_plot_marks(caps, np.array([(-8192, -8192, 16383, 16383, 0xFFFFFF)], dtype=engine.RECT), W, H)
    refused([(5, 0, 4, 1, 0)], match="x1 < x0 or y1 < y0")
    refused([(0, 5, 1, 4, 0)], match="x1 < x0 or y1 < y0")
    refused([(0, 0, 1, 1, 0x1000000)], match="colour beyond 0xFFFFFF")
    for bad in [(0, 0, 0, 20000, 1, 0, 255), (0, 0, 1, 1, 0, 0, 255), (0, 0, 1, 1, 1, 0, 0), (0, 0, 1, 1, 1, 0, 256), (0, 0, 1, 1, 1025, 0, 9), (0, 0, 1, 1, 1, 0x1000000, 9)]:
        refused(RECTS, caps=np.array([bad], dtype=engine.CAPSULE))
    refused(RECTS, w=9000)
    refused(RECTS, h=0)
    lib = L.lib()
    rects = np.array(RECTS, dtype=engine.RECT)
    out = np.zeros((H, W, 3), dtype=np.uint8)
    assert lib.ldw_debug_plot_marks(engine._ctx, L.ptr(caps), len(caps), None, 3, W, H, L.ptr(out), None) == L.LDW_ERR_ARG          # a null list
    assert lib.ldw_debug_plot_marks(engine._ctx, L.ptr(caps), len(caps), L.ptr(rects), len(rects), W, H, None, None) == L.LDW_ERR_ARG  # a null output
    assert lib.ldw_debug_plot_marks(None, L.ptr(caps), len(caps), L.ptr(rects), len(rects), W, H, L.ptr(out), None) == L.LDW_ERR_ARG
    xy = np.zeros((1, 2), dtype=np.int32)
    names = (C.c_char_p * 1)(b"a")
    args = (engine._ctx, L.ptr(caps), len(caps), L.ptr(rects), len(rects), W, H)
    assert lib.ldw_plot_tanglegram(*args, L.ptr(xy), C.cast(names, C.c_void_p), 1, b"t", 1, None, None, None) == L.LDW_ERR_ARG        # nowhere to write to
    for scale in (0, 65):
        assert lib.ldw_plot_tanglegram(*args, L.ptr(xy), C.cast(names, C.c_void_p), 1, b"t", scale, None, L.ptr(out), None) == L.LDW_ERR_ARG
    assert lib.ldw_plot_tanglegram(*args, None, None, 1, b"t", 1, None, L.ptr(out), None) == L.LDW_ERR_ARG
    null_name = (C.c_char_p * 1)(None)
    assert lib.ldw_plot_tanglegram(*args, L.ptr(xy), C.cast(null_name, C.c_void_p), 1, b"t", 1, None, L.ptr(out), None) == L.LDW_ERR_ARG
    assert lib.ldw_plot_tanglegram(*args, L.ptr(xy), C.cast(names, C.c_void_p), -1, b"t", 1, None, L.ptr(out), None) == L.LDW_ERR_ARG
    _same(engine, CAPS, RECTS)                                          # the context works on


def test_labels_and_title_boxes(engine):
    caps, rects = np.array(CAPS, dtype=engine.CAPSULE), np.array(RECTS, dtype=engine.RECT)
    w, h = 200, 120
    raster = engine.debug_plot_marks(caps, rects, w, h)
    xy = [(20, 100), (60, 110), (195, 30)]
    canvas, boxes = engine.plot_tanglegram(caps, rects, w, h, xy, ["abc", "", "edge"], "T 2", 1, want_canvas=True)
    assert boxes.tolist() == [[20, 100 - 17 + 1, 7, 17], [60, 110, 0, 0], [195, 30 - 23 + 1, 7, 23], [(w - 17) // 2, 2, 17, 7]]
    drawn = np.zeros((h, w), dtype=bool)
    for x, y, bw, bh in boxes.tolist():
        drawn[max(y, 0):max(y + bh, 0), max(x, 0):max(x + bw, 0)] = True
    assert np.array_equal(canvas[~drawn], raster[~drawn])
    for x, y, bw, bh in (boxes[0].tolist(), boxes[3].tolist()):        # ink in every box, up to its edges
        ink = (canvas[y:y + bh, x:x + bw] != raster[y:y + bh, x:x + bw]).any(axis=2)
        assert ink.any(axis=1)[[0, -1]].all() and ink.any(axis=0)[[0, -1]].all()
    # upwards: "abc" turned a quarter turn counter-clockwise is the horizontal text's transpose, mirrored top to bottom
    flat, _ = engine.plot_tanglegram(np.zeros(0, dtype=engine.CAPSULE), np.zeros(0, dtype=engine.RECT), 64, 64, [(10, 40)], ["abc"], "", 1, want_canvas=True)
    up = (flat[40 - 16:41, 10:17] != 255).any(axis=2)
    assert up.sum() > 20 and up[-1].any() and not (flat[:, :10] != 255).any()


def test_create_tanglegram_png(engine, tmp_path):
    th = make_tophits()
    assert len(th) == 60
    folder = tmp_path / "tng"
    got = T.create_tanglegram(th, gbk=record(*genome()), tanglegram_folder=str(folder), break_segments=3, plot_w=640, plot_h=400, engine=engine)
    assert sorted(os.listdir(folder)) == [f"tng_{g['segment']}.png" for g in got] == ["tng_1.png", "tng_2.png", "tng_3.png"]
    for g in got:
        dec, ihdr = R.png_decode(open(g["png"], "rb").read())
        assert dec.shape == (400, 640, 3) and ihdr[:2] == (640, 400) and g["png"] == str(folder / f"tng_{g['segment']}.png")
        want = TR.paint_marks(g["capsules"].tolist(), g["rects"].tolist(), 640, 400)
        n = len(g["labels"]["text"])
        boxes = g["boxes"]
        assert boxes.shape == (n + 1, 4) and boxes[-1, 2] > 0 and np.array_equal(boxes[:n], g["layout"]["label_box"])
        assert g["labels"]["drawn"].any() and (boxes[:n, 2] > 0).tolist() == g["labels"]["drawn"].tolist()
        drawn = np.zeros((400, 640), dtype=bool)
        for x, y, w, h in boxes.tolist():
            drawn[max(y, 0):max(y + h, 0), max(x, 0):max(x + w, 0)] = True
        assert np.array_equal(dec[~drawn], want[~drawn]) and (~drawn).sum() > 200000
        assert not np.array_equal(dec[drawn], want[drawn])              # the labels are there
        assert (want == (0xEE, 0, 0)).all(axis=2).any() and (want == (0x46, 0x82, 0xB4)).all(axis=2).any() and (want == 0xBE).all(axis=2).any()


def test_a_segment_without_links_writes_no_file(engine, tmp_path):
    import pandas as pd
    th = pd.DataFrame({"pos1": [1100, 5100, 40000, 40100], "pos1_genreg": ["G000", "G001", "G009-G010", "G009-G010"], "pos2_genreg": ["G001", "G002", "G010", "G011"],
                       "srp": [1.0, 3.0, 5.0, 6.0], "MI": [0.1] * 4})
    with pytest.warns(UserWarning):
        got = T.create_tanglegram(th, gbk=record(*genome(12)), tanglegram_folder=str(tmp_path), break_segments=2, plot_w=640, plot_h=400, engine=engine)
    assert os.listdir(tmp_path) == ["tng_1.png"] and "png" in got[0] and "png" not in got[1]
