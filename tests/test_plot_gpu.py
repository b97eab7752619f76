"""The device side of the plots (ldweaver_amd/csrc/ldw_plot.hip) against the numpy restatement of the rules in plot_ref.py:
every pixel of every panel must equal the naive painter's.  Needs an MI355X."""
import ctypes as C
import os

import numpy as np
import pytest

import plot_ref as R
from ldweaver_amd import _lib as L
from ldweaver_amd import plots as P

pytestmark = pytest.mark.gpu


def table(n, n_panels=1, seed=0, ties=False, one_pixel=False, layers="mixed", flat_srp=False, bad=False):
    rng = np.random.default_rng(seed)
    x = np.floor(rng.random(n) * 50000.0) + 1.0
    y = rng.random(n) ** 3
    srp = np.floor(rng.random(n) * 6) + 3.0 if ties else 3.0 + rng.exponential(2.0, n)
    if one_pixel:
        x[:], y[:] = 777.0, 0.25
    if flat_srp:
        srp[:] = 4.5
    layer = {"mixed": (rng.random(n) < 0.6), "zeros": np.zeros(n, bool), "ones": np.ones(n, bool)}[layers].astype(np.uint8)
    panel = rng.integers(0, n_panels, n).astype(np.uint8)
    if bad and n >= 8:
        x[1], y[2], srp[3], x[4], srp[5], srp[6], y[7] = np.nan, np.inf, np.nan, -np.inf, -1.0, -0.0, -0.0
    return x, y, srp, layer, panel


def reference(x, y, srp, layer, panel, n_panels, W, H, D, ordered, **kw):
    xr, yr = R.data_ranges(x, y, srp, kw.get("hline"))
    _, _, xt = P.ticks(xr[0], xr[1], W, False)
    _, _, yt = P.ticks(yr[0], yr[1], H, True)
    return R.naive_painter(x, y, srp, layer, panel, n_panels, W, H, D, ordered, xt, yt, **kw)


def to_device(cols):
    import torch
    return [None if c is None else torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in cols]


CASES = [
    dict(n=0), dict(n=1), dict(n=2), dict(n=2, n_panels=2), dict(n=300, n_panels=3, bad=True), dict(n=5000, n_panels=1), dict(n=5000, n_panels=2),
    dict(n=5000, n_panels=4, ties=True), dict(n=5000, n_panels=5), dict(n=5000, n_panels=6, D=3), dict(n=5000, n_panels=7, D=1),
    dict(n=5000, n_panels=8, D=21), dict(n=5000, n_panels=9, ties=True, D=21), dict(n=5000, n_panels=10, bad=True),
    dict(n=4000, one_pixel=True), dict(n=4000, one_pixel=True, ties=True, n_panels=3), dict(n=3000, layers="zeros"), dict(n=3000, layers="ones"),
    dict(n=3000, flat_srp=True), dict(n=3000, flat_srp=True, layers="ones", D=3), dict(n=200_000, n_panels=4, ties=True, D=3, bad=True),
    dict(n=5000, n_panels=2, D=41), dict(n=2_000_000, n_panels=3, W=640, H=400),      # (2e6 host rows: two chunks of the host-column feed)
]


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_exact_raster(engine, case, ordered):
    case = dict(case)
    D, W, H, n_panels = case.pop("D", 11), case.pop("W", 211), case.pop("H", 97), case.get("n_panels", 1)
    x, y, srp, layer, panel = table(seed=len(CASES) + case["n"] + D, **case)
    want = reference(x, y, srp, layer, panel, n_panels, W, H, D, ordered)
    o = P.plot_opts(L.PLOT_SR_CLUST, D, ordered)
    got, st, scratch, _ = P.debug_panels(engine, x, y, srp, layer, panel, opts=o, n_panels=n_panels, W=W, H=H)
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).any(axis=-1).sum())} pixels differ"
    keep = R.keep_mask(x, y, srp)
    assert st["kept"] == int(keep.sum()) and st["dropped"] == int((~keep).sum())
    assert scratch <= 11 * n_panels * W * H + 131072
    dev, _, _, _ = P.debug_panels(engine, *to_device([x, y, srp, layer, panel]), opts=o, n_panels=n_panels, W=W, H=H)
    assert np.array_equal(dev, want)
    # the pre-check load is an optimisation only
    o2 = P.plot_opts(L.PLOT_SR_CLUST, D, ordered, no_precheck=True)
    assert np.array_equal(P.debug_panels(engine, x, y, srp, layer, panel, opts=o2, n_panels=n_panels, W=W, H=H)[0], want)


def test_fixed_colours_and_line(engine):
    x, y, _, layer, _ = table(6000, seed=3)
    thr = float(np.quantile(y, 0.9))
    for hline in (None, thr, 2.0 * y.max()):           # (a line above every point widens the y range)
        kw = dict(layer_rgb=(P.GREY, P.LR_DIRECT), hline=hline, hline_rgb=P.LR_LINE)
        want = reference(x, y, None, layer, None, 1, 400, 150, 11, False, **kw)
        got = P.debug_panels(engine, x, y, None, layer, None, opts=P.plot_opts(L.PLOT_LR, 11, **kw), W=400, H=150)[0]
        assert np.array_equal(got, want)
        if hline is not None:
            lim = R.axis_range(*R.data_ranges(x, y, None, hline)[1])
            assert (got[0, 149 - int(R.pixel(hline, lim[0], lim[1], 150))] == R.rgb_of(P.LR_LINE)).all()
    black = P.debug_panels(engine, x, y, opts=P.plot_opts(L.PLOT_LR, 11, layer_rgb=(0, 0)), W=400, H=150)[0]
    assert np.array_equal(black, reference(x, y, None, None, None, 1, 400, 150, 11, False, layer_rgb=(0, 0)))


def test_refusals(engine, tmp_path):
    lib = L.lib()
    x, y, srp, layer, panel = table(100, n_panels=3, seed=1)
    rgb = np.zeros((3, 16, 16, 3), dtype=np.uint8)
    ctx = engine._ctx

    def call(x=x, y=y, srp=srp, layer=layer, panel=panel, n=100, o=None, n_panels=3, W=16, H=16):
        o = o or P.plot_opts(L.PLOT_SR_CLUST)
        return lib.ldw_debug_plot_panels(ctx, L.ptr(x), L.ptr(y), L.ptr(srp), L.ptr(layer), L.ptr(panel), n, 0, C.byref(o), n_panels, W, H, L.ptr(rgb),
                                         None, None, None)
    assert call() == L.LDW_OK
    assert call(x=None) == L.LDW_ERR_ARG and call(y=None) == L.LDW_ERR_ARG and call(n=-1) == L.LDW_ERR_ARG
    for D in (2, 10, -1, 43):
        assert call(o=P.plot_opts(L.PLOT_SR_CLUST, D)) == L.LDW_ERR_ARG, D
    assert call(n_panels=2) == L.LDW_ERR_ARG and "panel id" in lib.ldw_last_error().decode()       # ids 0..2 with two panels
    assert call(n_panels=0) == L.LDW_ERR_ARG and call(n_panels=11) == L.LDW_ERR_ARG and call(W=0) == L.LDW_ERR_ARG
    assert call(srp=None, o=P.plot_opts(L.PLOT_SR_CLUST, 11, True)) == L.LDW_ERR_ARG                # row order needs srp
    assert call(o=P.plot_opts(L.PLOT_LDMAP)) == L.LDW_ERR_ARG
    o = P.plot_opts(L.PLOT_SR_COMBI)
    bad = os.fsencode(tmp_path / "missing" / "a.png")
    assert lib.ldw_plot_scatter(ctx, L.ptr(x), L.ptr(y), L.ptr(srp), L.ptr(layer), None, 100, 0, C.byref(o), 1, None, bad, None, None) == L.LDW_ERR_ARG
    assert "missing" in lib.ldw_last_error().decode()
    assert lib.ldw_plot_scatter(ctx, L.ptr(x), L.ptr(y), L.ptr(srp), L.ptr(layer), None, 100, 0, C.byref(o), 1, None, None, None, None) == L.LDW_ERR_ARG
    assert lib.ldw_plot_scatter(ctx, L.ptr(x), L.ptr(y), L.ptr(srp), L.ptr(layer), None, 100, 0, C.byref(o), 2, None, bad, None, None) == L.LDW_ERR_ARG
    assert lib.ldw_plot_heatmap(ctx, None, 4, 0, None, bad, None) == L.LDW_ERR_ARG
    assert lib.ldw_plot_heatmap(ctx, L.ptr(x), 0, 0, None, bad, None) == L.LDW_ERR_ARG


def test_order_independence(engine, tmp_path):
    x, y, srp, layer, panel = table(150_000, n_panels=6, seed=9, ties=True)
    labels = np.arange(1, 7)
    o = P.plot_opts(L.PLOT_SR_CLUST)
    P.render_scatter(engine, x, y, srp, layer, panel, opts=o, n_panels=6, labels=labels, path=tmp_path / "a.png")
    P.render_scatter(engine, x, y, srp, layer, panel, opts=o, n_panels=6, labels=labels, path=tmp_path / "b.png")
    perm = np.random.default_rng(1).permutation(len(x))
    P.render_scatter(engine, x[perm], y[perm], srp[perm], layer[perm], panel[perm], opts=o, n_panels=6, labels=labels, path=tmp_path / "c.png")
    a = (tmp_path / "a.png").read_bytes()
    assert a == (tmp_path / "b.png").read_bytes() and a == (tmp_path / "c.png").read_bytes()


def panels_of(canvas, lay):
    return np.stack([canvas[y:y + h, x:x + w] for (x, y, w, h) in lay["panels"]])


def test_frame(engine, tmp_path):
    x, y, srp, layer, panel = table(20_000, n_panels=5, seed=4)
    labels = np.array([1, 2, 3, 5, 8], dtype=np.int32)
    for kind, n_panels, pan in ((L.PLOT_SR_CLUST, 5, panel), (L.PLOT_SR_COMBI, 1, None), (L.PLOT_LR, 1, None)):
        lr = kind == L.PLOT_LR
        o = P.plot_opts(kind, layer_rgb=(P.GREY, P.LR_DIRECT))
        path = tmp_path / f"k{kind}.png"
        canvas, _ = P.render_scatter(engine, x, y, None if lr else srp, layer, pan, opts=o, n_panels=n_panels, labels=labels[:n_panels], path=path,
                                     want_canvas=True)
        dec, _ = R.png_decode(path.read_bytes())
        assert np.array_equal(dec, canvas) and canvas.shape[:2] == P.CANVAS[kind][::-1]
        xr, yr = R.data_ranges(x, y, None if lr else srp)
        lay = P.layout(kind, n_panels, xr, yr)
        want = R.naive_painter(x, y, None if lr else srp, layer, pan, n_panels, lay["panel_w"], lay["panel_h"], 11, False, lay["xtick_px"], lay["ytick_px"],
                               layer_rgb=(P.GREY, P.LR_DIRECT) if lr else None)
        assert np.array_equal(panels_of(canvas, lay), want)
        # outside the panels, the strips and the colour bar: the frame's declared colours only
        mask = np.ones(canvas.shape[:2], dtype=bool)
        for (rx, ry, rw, rh) in lay["panels"] + lay["strips"] + ([lay["cbar"]] if lay["cbar"] else []):
            mask[ry:ry + rh, rx:rx + rw] = False
        pix = canvas[mask].astype(np.int64)
        packed = (pix[:, 0] << 16) | (pix[:, 1] << 8) | pix[:, 2]
        allowed = {(r << 16) | (g << 8) | b for (r, g, b) in P.FRAME_COLOURS}
        assert set(np.unique(packed).tolist()) <= allowed
        assert len(set(np.unique(packed).tolist())) >= 3          # (lines, labels and titles were drawn)
        # ink at every tick mark: left of the first column's panels, under the bottom panels
        border = P.FRAME_COLOURS[1]
        for k, (px_, py_, pw, ph) in enumerate(lay["panels"]):
            if k % lay["cols"] == 0:
                for t in lay["ytick_px"]:
                    assert tuple(canvas[py_ + t, px_ - 3]) == border
            if k + lay["cols"] >= n_panels:
                for t in lay["xtick_px"]:
                    assert tuple(canvas[py_ + ph + 3, px_ + t]) == border
        if lay["cbar"]:
            cx, cy, cw, ch = lay["cbar"]
            assert tuple(canvas[cy, cx]) == (0xD7, 0x30, 0x27) and tuple(canvas[cy + ch - 1, cx + cw - 1]) == (0x45, 0x75, 0xB4)


def test_heatmap(engine, tmp_path):
    rng = np.random.default_rng(2)
    for B in (1, 7, 333, 1000):
        htm = rng.random((B, B))
        htm = (htm + htm.T) / 2
        htm.flat[:: max(B * B // 50, 1)] = [0.0, 1.0, np.nan, 0.5, np.nextafter(1.0, 0)][B % 5]
        P.render_heatmap(engine, htm, tmp_path / "h.png", title=f"LD map {B}")
        dec, ihdr = R.png_decode((tmp_path / "h.png").read_bytes())
        assert ihdr[:2] == (5000, 5250)
        lay = P.layout(L.PLOT_LDMAP)
        assert np.array_equal(panels_of(dec, lay)[0], R.heat_raster(htm, lay["panel_w"], lay["panel_h"]))
        import torch
        P.render_heatmap(engine, torch.from_numpy(htm).cuda(), tmp_path / "hd.png", title=f"LD map {B}")
        assert (tmp_path / "hd.png").read_bytes() == (tmp_path / "h.png").read_bytes()


def test_from_the_engine(tmp_path, synth):
    """perform_MI_computation leaves the kept links on the device: the figures rendered from there equal those of the returned frame, and
    both equal the naive painter; the same for the long-range figure with its threshold line and for the LD map."""
    from ldweaver_amd import lr as LR
    from ldweaver_amd import mi as MIH
    from ldweaver_amd.engine import Engine
    from ldweaver_amd.snpdat import CdsVar, SnpDat
    st, POS = synth["states"], synth["POS"]
    sd = SnpDat.from_states(st, POS, g=synth["g"])
    cv = CdsVar(paint=synth["paint"], nclust=int(synth["paint"].max()))
    with Engine(0) as eng:
        eng.set_alignment(st)
        red = MIH.perform_MI_computation(sd, synth["hdw"], cv, lr_save_path=str(tmp_path / "lr.tsv"), sr_save_path=str(tmp_path / "sr.tsv"),
                                         plt_folder=str(tmp_path / "P"), sr_dist=50000, engine=eng, alignment_resident=True, verbose=False)
        assert len(red) > 10
        a = P.make_gwes_plots(engine=eng, plt_folder=str(tmp_path / "E"))
        b = P.make_gwes_plots(sr_links=red, plt_folder=str(tmp_path / "F"), engine=eng)
        c = P.make_gwes_plots(sr_links=str(tmp_path / "sr.tsv"), lr_links=str(tmp_path / "lr.tsv"), plt_folder=str(tmp_path / "G"), engine=eng)
        assert sorted(a) == sorted(b) == ["sr_gwes_clust", "sr_gwes_combi"] and sorted(c) == ["lr_gwes", "sr_gwes_clust", "sr_gwes_combi"]
        x, y, srp = red["len"].to_numpy(float), red["MI"].to_numpy(float), red["srp_max"].to_numpy(float)
        layer = (red["ARACNE"].to_numpy() != 0).astype(np.uint8)
        panel, labels = P.sr_facets(red["clust_c"].to_numpy())
        xr, yr = R.data_ranges(x, y, srp)
        for name, kind, n_panels, pan in (("sr_gwes_clust", L.PLOT_SR_CLUST, len(labels), panel), ("sr_gwes_combi", L.PLOT_SR_COMBI, 1, None)):
            data = open(a[name], "rb").read()
            assert data == open(b[name], "rb").read()
            assert R.png_decode(open(c[name], "rb").read())[1][:2] == (2200, 1200)     # (the tsv holds 15 significant digits: not the same table)
            dec, ihdr = R.png_decode(data)
            assert ihdr[:2] == (2200, 1200)
            lay = P.layout(kind, n_panels, xr, yr)
            want = R.naive_painter(x, y, srp, layer, pan, n_panels, lay["panel_w"], lay["panel_h"], 11, False, lay["xtick_px"], lay["ytick_px"])
            assert np.array_equal(panels_of(dec, lay), want)
        # row order as the draw order: from the frame only
        o = P.make_gwes_plots(sr_links=red, plt_folder=str(tmp_path / "O"), are_srlinks_ordered=True, engine=eng)
        lay = P.layout(L.PLOT_SR_COMBI, 1, xr, yr)
        want = R.naive_painter(x, y, srp, layer, None, 1, lay["panel_w"], lay["panel_h"], 11, True, lay["xtick_px"], lay["ytick_px"])
        assert np.array_equal(panels_of(R.png_decode(open(o["sr_gwes_combi"], "rb").read())[0], lay), want)
        with pytest.raises(ValueError, match="are_srlinks_ordered"):
            P.make_gwes_plots(engine=eng, plt_folder=str(tmp_path / "E"), are_srlinks_ordered=True)
        # lr_gwes.png of make_gwes_plots: one black layer over the whole lr table
        lrt = P.read_LongRangeLinks(str(tmp_path / "lr.tsv"))
        lx, ly = lrt["len"].to_numpy(float), lrt["MI"].to_numpy(float)
        lay = P.layout(L.PLOT_LR, 1, *R.data_ranges(lx, ly))
        dec, ihdr = R.png_decode(open(c["lr_gwes"], "rb").read())
        assert ihdr[:2] == (4800, 1200)
        want = R.naive_painter(lx, ly, None, None, None, 1, lay["panel_w"], lay["panel_h"], 11, False, lay["xtick_px"], lay["ytick_px"], layer_rgb=(0, 0))
        assert np.array_equal(panels_of(dec, lay), want)
        # analyse_long_range_links: grey under blue, the line at max(thresholds)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            plain = LR.analyse_long_range_links(eng, sd, red, cv)
            out = LR.analyse_long_range_links(eng, sd, red, cv, lr_plt_path=str(tmp_path / "lr_gwes.png"))
        df = out["lr_links_red"]
        assert df.equals(plain["lr_links_red"]) and len(df) > 0
        thr = float(np.max(out["thresholds"]))
        lx, ly, ll = df["len"].to_numpy(float), df["MI"].to_numpy(float), (df["ARACNE"].to_numpy() != 0).astype(np.uint8)
        lay = P.layout(L.PLOT_LR, 1, *R.data_ranges(lx, ly, None, thr))
        want = R.naive_painter(lx, ly, None, ll, None, 1, lay["panel_w"], lay["panel_h"], 11, False, lay["xtick_px"], lay["ytick_px"],
                               layer_rgb=(P.GREY, P.LR_DIRECT), hline=thr, hline_rgb=P.LR_LINE)
        got = panels_of(R.png_decode((tmp_path / "lr_gwes.png").read_bytes())[0], lay)
        assert np.array_equal(got, want)
        row = lay["panel_h"] - 1 - int(R.pixel(thr, lay["ylim"][0], lay["ylim"][1], lay["panel_h"]))
        assert (got[0, row] == R.rgb_of(P.LR_LINE)).all()
        # the LD map
        m0 = LR.genomewide_LDMap(eng, sd, reducer=7)
        m1 = LR.genomewide_LDMap(eng, sd, reducer=7, plot_save_path=str(tmp_path / "LD_plot.png"), plot_title="synth")
        # (the map's block sums are floating-point atomic adds: two runs agree to rounding, not to the bit; the picture is that of m1's map)
        assert np.allclose(m0["htm"], m1["htm"], rtol=1e-9, atol=1e-12, equal_nan=True) and m0["n_pos"] == m1["n_pos"] and m0["reducer"] == m1["reducer"]
        dec, ihdr = R.png_decode((tmp_path / "LD_plot.png").read_bytes())
        assert ihdr[:2] == (5000, 5250)
        lay = P.layout(L.PLOT_LDMAP)
        assert np.array_equal(panels_of(dec, lay)[0], R.heat_raster(m1["htm"], lay["panel_w"], lay["panel_h"]))
        title_band = dec[:lay["panels"][0][1] - 2]
        assert (title_band == 0).all(axis=-1).any() and set(np.unique(title_band).tolist()) == {0, 255}


def test_links_state_refusals(tmp_path, synth):
    """ldw_plot_links answers LDW_ERR_STATE, never a picture from stale memory: without SNP meta data, for the table whose links are not the
    kept ones, and with use_aracne when ldw_aracne_device has not run for the CURRENT kept links (ARACNE skipped, a new ldw_sr_pvalues, or
    ldw_lr_tukey, which also borrows the flags' buffer)."""
    from ldweaver_amd import mi as MIH
    from ldweaver_amd.engine import Engine
    from ldweaver_amd.snpdat import CdsVar, SnpDat
    lib = L.lib()
    o_sr, o_lr = P.plot_opts(L.PLOT_SR_COMBI), P.plot_opts(L.PLOT_LR, layer_rgb=(P.GREY, P.LR_DIRECT))

    def links(eng, which, use_aracne, o):
        return lib.ldw_plot_links(eng._ctx, which, use_aracne, C.byref(o), os.fsencode(tmp_path / "s.png"), None, None)
    st, POS = synth["states"], synth["POS"]
    sd = SnpDat.from_states(st, POS, g=synth["g"])
    cv = CdsVar(paint=synth["paint"], nclust=int(synth["paint"].max()))
    kw = dict(lr_save_path=str(tmp_path / "lr.tsv"), sr_save_path=str(tmp_path / "sr.tsv"), plt_folder=str(tmp_path / "P"), sr_dist=50000,
              alignment_resident=True, verbose=False)
    with Engine(0) as eng:
        assert links(eng, 0, 0, o_sr) == L.LDW_ERR_STATE and "ldw_set_snp_meta" in lib.ldw_last_error().decode()
        eng.set_alignment(st)
        red = MIH.perform_MI_computation(sd, synth["hdw"], cv, engine=eng, runARACNE=False, **kw)
        assert len(red) > 10 and (red["ARACNE"] == 1).all()
        assert links(eng, 0, 1, o_sr) == L.LDW_ERR_STATE and "ldw_aracne_device" in lib.ldw_last_error().decode()
        assert links(eng, 1, 0, o_lr) == L.LDW_ERR_STATE          # the kept links are short-range ones
        assert links(eng, 0, 1, o_lr) == L.LDW_ERR_ARG            # figure kind and table do not fit
        with pytest.raises(L.LdwError) as e:
            P.make_gwes_plots(engine=eng, plt_folder=str(tmp_path / "E"))
        assert e.value.code == L.LDW_ERR_STATE
        a = P.make_gwes_plots(engine=eng, plt_folder=str(tmp_path / "E"), aracne=False)      # every link direct, like the frame's column of ones
        b = P.make_gwes_plots(sr_links=red, plt_folder=str(tmp_path / "F"), engine=eng)
        for k in a:
            assert open(a[k], "rb").read() == open(b[k], "rb").read()
        # ARACNE run, then the kept set replaced: the flags on the device belong to the old set
        (tmp_path / "lr.tsv").unlink()
        red = MIH.perform_MI_computation(sd, synth["hdw"], cv, engine=eng, **kw)
        assert links(eng, 0, 1, o_sr) == L.LDW_OK
        from ldweaver_amd.lr import positions_to_snp_index
        a_, b_ = positions_to_snp_index(POS, red["pos2"].to_numpy()), positions_to_snp_index(POS, red["pos1"].to_numpy())
        info = eng.lr_tukey(5000, sr=(a_, b_, red["MI"].to_numpy(float)))
        assert info["n_red"] > 0
        assert links(eng, 1, 1, o_lr) == L.LDW_ERR_STATE and "ldw_aracne_device" in lib.ldw_last_error().decode()
        assert links(eng, 0, 0, o_sr) == L.LDW_ERR_STATE          # the kept links are long-range ones now
        assert links(eng, 1, 0, o_lr) == L.LDW_OK
        eng.aracne_device()
        assert links(eng, 1, 1, o_lr) == L.LDW_OK
    with pytest.raises(TypeError, match="one Engine"):
        P.render_links(object(), 0, opts=o_sr, path=tmp_path / "t.png")


def test_scale(engine):
    """1e8 rows generated on the device and rendered from device pointers for the 2200 x 1200 combined figure's panel.  The test reduces the
    same columns (fetched in chunks of 1e7 rows) with numpy's maximum.at to the per-pixel maximum of the key, keeps one row per winning
    pixel and feeds those to the naive painter.  Scratch memory does not depend on n."""
    import torch
    lay = P.layout(L.PLOT_SR_COMBI)
    W, H = lay["panel_w"], lay["panel_h"]
    o = P.plot_opts(L.PLOT_SR_COMBI)
    scratch = {}
    for n in (1_000_000, 100_000_000):
        gen = torch.Generator(device="cuda").manual_seed(n % 1000 + 5)
        x = torch.floor(torch.rand(n, generator=gen, device="cuda", dtype=torch.float64) * 50000.0) + 1.0
        y = torch.rand(n, generator=gen, device="cuda", dtype=torch.float64) ** 4
        srp = 3.0 + torch.floor(-4000.0 * torch.log1p(-torch.rand(n, generator=gen, device="cuda", dtype=torch.float64))) / 1000.0   # ties
        layer = (torch.rand(n, generator=gen, device="cuda") < 0.7).to(torch.uint8)
        got, st, scratch[n], _ = P.debug_panels(engine, x, y, srp, layer, None, opts=o, W=W, H=H)
        assert st["kept"] == n and st["dropped"] == 0
        direct = srp[layer != 0]
        assert st["xr"] == (float(x.min()), float(x.max())) and st["yr"] == (float(y.min()), float(y.max()))
        assert (st["lo"], st["hi"]) == (float(direct.min()), float(direct.max()))
        del direct
        assert scratch[n] <= 8 * W * H + 3 * W * H + 131072
        x0, x1 = R.axis_range(*st["xr"])
        y0, y1 = R.axis_range(*st["yr"])
        img = np.zeros(W * H, dtype=np.uint64)
        step = 10_000_000
        keys = lambda s_, l_: ((l_.astype(np.uint64) << np.uint64(63)) | s_.view(np.uint64)) + np.uint64(1)
        for a in range(0, n, step):
            cx, cy, cs, cl = (t[a:a + step].cpu().numpy() for t in (x, y, srp, layer))
            at = (H - 1 - R.pixel(cy, y0, y1, H)) * W + R.pixel(cx, x0, x1, W)
            np.maximum.at(img, at, keys(cs, cl))
        rx, ry, rs, rl = [], [], [], []
        seen = np.zeros(W * H, dtype=bool)
        for a in range(0, n, step):
            cx, cy, cs, cl = (t[a:a + step].cpu().numpy() for t in (x, y, srp, layer))
            at = (H - 1 - R.pixel(cy, y0, y1, H)) * W + R.pixel(cx, x0, x1, W)
            win = np.flatnonzero((keys(cs, cl) == img[at]) & ~seen[at])
            _, first = np.unique(at[win], return_index=True)       # one row per winning pixel
            win = win[first]
            seen[at[win]] = True
            rx.append(cx[win]); ry.append(cy[win]); rs.append(cs[win]); rl.append(cl[win])
        rx, ry, rs, rl = (np.concatenate(v) for v in (rx, ry, rs, rl))
        assert len(rx) == int((img != 0).sum()) <= W * H
        _, _, xt = P.ticks(st["xr"][0], st["xr"][1], W, False)
        _, _, yt = P.ticks(st["yr"][0], st["yr"][1], H, True)
        want = R.naive_painter(rx, ry, rs, rl, None, 1, W, H, 11, False, xt, yt, ranges=(st["xr"], st["yr"]), srp_range=(st["lo"], st["hi"]))
        assert np.array_equal(got, want), f"n = {n}: {int((got != want).any(axis=-1).sum())} pixels differ"
        del x, y, srp, layer
        torch.cuda.empty_cache()
    assert scratch[1_000_000] == scratch[100_000_000]
