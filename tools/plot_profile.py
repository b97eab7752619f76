"""Times of the plot kernels (hip events inside ldw_debug_plot_panels) for the 2200 x 1200 combined figure, a plain device copy of the same
bytes as the yardstick, and make_gwes_plots file to file at 1e7 rows.  Needs an MI355X.

    python tools/plot_profile.py [OUT.json] [SCRATCH_DIR]      (defaults: profiles/plot_render.json, a temporary directory)

Every host timer below encloses a synchronise (the library's calls return after theirs)."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "plot_render.json")
import tempfile   # noqa: E402
TMP = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="ldw_plot_")
sys.path.insert(0, ROOT)
from ldweaver_amd import _lib as L          # noqa: E402
from ldweaver_amd import plots as P         # noqa: E402
from ldweaver_amd.engine import Engine, write_table_tsv   # noqa: E402

out = {"figure": "sr_gwes_combi 2200 x 1200", "D": 11, "bytes_per_row": 25, "runs": []}
lay = P.layout(L.PLOT_SR_COMBI)
W, H = lay["panel_w"], lay["panel_h"]
out["panel"] = [W, H]


def med(v):
    return float(np.median(v))


with Engine(0) as eng:
    for n in (1_000_000, 10_000_000, 100_000_000):
        gen = torch.Generator(device="cuda").manual_seed(7)
        x = torch.floor(torch.rand(n, generator=gen, device="cuda", dtype=torch.float64) * 50000.0) + 1.0
        y = torch.rand(n, generator=gen, device="cuda", dtype=torch.float64) ** 4
        srp = 3.0 - 4.0 * torch.log1p(-torch.rand(n, generator=gen, device="cuda", dtype=torch.float64))
        layer = (torch.rand(n, generator=gen, device="cuda") < 0.7).to(torch.uint8)
        rec = {"n": n}
        for name, kw in (("precheck", {}), ("no_precheck", dict(no_precheck=True)), ("row_order", dict(ordered=True))):
            o = P.plot_opts(L.PLOT_SR_COMBI, **kw)
            ms = []
            for rep in range(5):
                _, st, scratch, t = P.debug_panels(eng, x, y, srp, layer, None, opts=o, W=W, H=H, timing=True)
                if rep >= 2:
                    ms.append(t)
            rec[name] = {k: med([m[k] for m in ms]) for k in ms[0]}
            rec["scratch_bytes"] = scratch
        # yardstick: a plain device copy of the 25 n bytes the centre pass reads
        src = torch.empty(25 * n, dtype=torch.uint8, device="cuda").random_(0, 255)
        dst = torch.empty_like(src)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        cp = []
        for rep in range(5):
            ev[0].record()
            dst.copy_(src)
            ev[1].record()
            torch.cuda.synchronize()
            if rep >= 2:
                cp.append(ev[0].elapsed_time(ev[1]))
        rec["copy_ms"] = med(cp)
        rec["copy_read_GBps"] = 25 * n / (med(cp) * 1e-3) / 1e9
        rec["centre_read_GBps"] = 25 * n / (rec["precheck"]["centre"] * 1e-3) / 1e9
        rec["centre_read_GBps_no_precheck"] = 25 * n / (rec["no_precheck"]["centre"] * 1e-3) / 1e9
        out["runs"].append(rec)
        print(json.dumps(rec), flush=True)
        del src, dst
        if n == 10_000_000:
            # make_gwes_plots file to file, and where the time of ONE figure (sr_gwes_combi.png) from host columns goes
            os.makedirs(TMP, exist_ok=True)
            path = os.path.join(TMP, "sr_1e7.tsv")
            hx, hy, hs, hl = x.cpu().numpy(), y.cpu().numpy(), srp.cpu().numpy(), layer.cpu().numpy()
            clust = (np.arange(n) % 3 + 1).astype(np.int32)
            cols = [clust, hx.astype(np.int32), hx.astype(np.int32), clust, clust, hx, hy, hs, hl.astype(np.int32)]
            if os.path.exists(path):
                os.remove(path)
            write_table_tsv(path, cols, append=False)
            f2f = {"rows": n, "tsv_bytes": os.path.getsize(path)}
            t0 = time.time()
            df = P.read_ShortRangeLinks(path)
            f2f["tsv_read_s"] = time.time() - t0
            P.make_gwes_plots(sr_links=df, plt_folder=os.path.join(TMP, "WARM"), engine=eng)      # (first use: buffers, code objects)
            t0 = time.time()
            res = P.make_gwes_plots(sr_links=df, plt_folder=os.path.join(TMP, "PLOTS"), engine=eng)
            f2f["make_gwes_plots_two_figures_s"] = time.time() - t0
            t0 = time.time()
            panel, labels = P.sr_facets(df["clust_c"].to_numpy())
            f2f["facets_np_unique_s"] = time.time() - t0
            t0 = time.time()
            a = [np.ascontiguousarray(df[c].to_numpy(), dtype=np.float64) for c in ("len", "MI", "srp_max")] + [(df["ARACNE"].to_numpy() != 0).astype(np.uint8)]
            f2f["frame_to_columns_s"] = time.time() - t0
            o = P.plot_opts(L.PLOT_SR_COMBI)
            P.debug_panels(eng, *a, None, opts=o, W=W, H=H)
            t0 = time.time()
            P.debug_panels(eng, *a, None, opts=o, W=W, H=H)          # host columns: chunked upload + the passes + rasters back
            f2f["upload_and_render_host_columns_s"] = time.time() - t0
            d = [torch.from_numpy(v).cuda() for v in a]
            torch.cuda.synchronize()
            t0 = time.time()
            P.debug_panels(eng, *d, None, opts=o, W=W, H=H)          # device columns: the passes + rasters back
            f2f["render_device_columns_s"] = time.time() - t0
            f2f["upload_s"] = f2f["upload_and_render_host_columns_s"] - f2f["render_device_columns_s"]
            f2f["upload_GBps"] = 25 * n / f2f["upload_s"] / 1e9
            t0 = time.time()
            canvas, _ = P.render_scatter(eng, *d, None, opts=o, want_canvas=True)
            f2f["render_plus_frame_s"] = time.time() - t0
            f2f["frame_s"] = f2f["render_plus_frame_s"] - f2f["render_device_columns_s"]
            t0 = time.time()
            f2f["png_bytes"] = P.png_write(os.path.join(TMP, "combi.png"), canvas)
            f2f["deflate_and_write_s"] = time.time() - t0
            f2f["png_sizes"] = [os.path.getsize(k) for k in res.values()]
            os.remove(path)
            out["file_to_file_1e7"] = f2f
            print(json.dumps(f2f), flush=True)
            del df, a, d, canvas
        del x, y, srp, layer
        torch.cuda.empty_cache()

with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
print("done")
