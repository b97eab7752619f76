"""Stage times of the five figure renderers from the library's own hip events, as raw repetitions, for comparing two builds of the library
(DESIGN.md 20).  Needs an MI355X.

    python tools/plot_ab.py run SIDE GROUP LINES.jsonl      one process: the build that LDW_AMD_LIB names (default: the tree's) as SIDE
    python tools/plot_ab.py merge LINES.jsonl OUT.json      (default OUT: profiles/plot_primitives_ab.json)

GROUP: scatter (tools/plot_profile.py's figure at 1e6 / 1e7 / 1e8 rows), xy (tools/driver_profile.py's two panels), network
(tools/network_profile.py's render step), tanglegram (the largest list of tests/test_tanglegram_gpu.py), tree (tools/tree_profile.py's cases).
A run makes 2 warm-up calls and 3 timed ones per case and appends one line per case; the caller alternates the sides, process by process.
merge: a stage passes when side "branch"'s median is no higher than the largest single value of side "parent"."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
WARM, REPS = 2, 3


def reps(call):
    """call() -> {stage: ms}; the timed calls' values per stage."""
    got = [call() for _ in range(WARM + REPS)][WARM:]
    return {k: [round(float(g[k]), 5) for g in got] for k in got[0]}


def group_scatter(eng):
    import torch
    from ldweaver_amd import _lib as L, plots as P
    lay = P.layout(L.PLOT_SR_COMBI)
    W, H = lay["panel_w"], lay["panel_h"]
    for n in (1_000_000, 10_000_000, 100_000_000):
        gen = torch.Generator(device="cuda").manual_seed(7)
        x = torch.floor(torch.rand(n, generator=gen, device="cuda", dtype=torch.float64) * 50000.0) + 1.0
        y = torch.rand(n, generator=gen, device="cuda", dtype=torch.float64) ** 4
        srp = 3.0 - 4.0 * torch.log1p(-torch.rand(n, generator=gen, device="cuda", dtype=torch.float64))
        layer = (torch.rand(n, generator=gen, device="cuda") < 0.7).to(torch.uint8)
        for name, kw in (("precheck", {}), ("no_precheck", dict(no_precheck=True)), ("row_order", dict(ordered=True))):
            o = P.plot_opts(L.PLOT_SR_COMBI, **kw)
            yield f"{n} rows, {name}", reps(lambda: P.debug_panels(eng, x, y, srp, layer, None, opts=o, W=W, H=H, timing=True)[3])
        del x, y, srp, layer
        torch.cuda.empty_cache()


def group_xy(eng):
    from ldweaver_amd import _lib as L, plots as P
    lay = P.layout(L.PLOT_FIT)
    W, H = lay["panel_w"], lay["panel_h"]
    rng = np.random.default_rng(3)
    for n, nv in ((100_000, 100_000), (5_000, 0)):
        ln = np.arange(1.0, n + 1)
        mx = 0.3 * np.exp(-ln / (n / 5)) + 0.03 + rng.normal(0, 0.004, n)
        line = (ln[:nv], (0.3 * np.exp(-ln / (n / 5)) + 0.03)[:nv]) if nv else None
        cls = None if nv else rng.integers(0, 3, n).astype(np.uint8)
        o = P.xy_opts(L.PLOT_FIT if nv else L.PLOT_CDS, class_rgb=[0] if nv else [0xF8766D, 0x00BA38, 0x619CFF])
        yield f"{n} points, {nv} vertices", reps(lambda: P.debug_xy_panel(eng, ln, mx, cls, line, opts=o, W=W, H=H, timing=True)[2])


def group_network(eng):
    import pandas as pd
    from ldweaver_amd import network as N
    rng = np.random.default_rng(1)
    k = 1000
    a = rng.integers(0, 400, k)
    b = (a + 1 + rng.integers(0, 398, k)) % 400
    e = pd.DataFrame({"p1": [f"g{i}" for i in a], "p2": [f"g{i}" for i in b], "Num_Links": rng.integers(2, 9, k), "weights": rng.random(k)})
    names, xy, _ = N.network_layout(e, 6000, 4000)
    caps, _, _ = N.network_capsules(e, names, xy, 6000)
    yield f"{len(caps)} capsules, 6000 x 4000", reps(lambda: dict(zip(("binning", "shading"), eng.plot_capsules(caps, 6000, 4000, timings=True)[1])))


def group_tanglegram(eng):
    W, H = 97, 70      # tests/test_tanglegram_gpu.py::test_many_rectangles_more_than_one_block
    rng = np.random.default_rng(8)
    caps = [(3, 20, 92, 20, 3, 0xFF0000, 200), (40, 2, 40, 68, 4, 0x00FF00, 128), (5, 5, 90, 66, 5, 0x0000FF, 90)]
    rects = [(0, 10, W, 14, 0x111111), (3, 0, 90, H, 0x222222)]
    for _ in range(3000):
        x, y = int(rng.integers(-4, W)), int(rng.integers(-4, H))
        rects.append((x, y, x + int(rng.integers(0, 6)), y + int(rng.integers(0, 6)), int(rng.integers(0, 1 << 24))))
    caps, rects = np.array(caps, dtype=eng.CAPSULE), np.array(rects, dtype=eng.RECT)
    yield f"{len(caps)} capsules, {len(rects)} rectangles, {W} x {H}", reps(
        lambda: dict(zip(("binning", "shading", "rectangles"), eng.debug_plot_marks(caps, rects, W, H, timings=True)[1])))


def group_tree(eng):
    import tree_profile as TP
    from ldweaver_amd import tree as T
    for n in TP.SIZES:
        for kind in TP.KINDS:
            rng = np.random.default_rng(n)
            tree = T.ladderize(T.midpoint_root(T.parse_newick(TP.newick(kind, n, rng).encode())))
            lay = T.tree_layout(tree, TP.W, TP.H, 0, TP.BANDS, band_labels=["1234567"] * TP.BANDS, legends=[("Metadata", [], []), ("Alleles", list("ACGTN"), [0] * 5)])
            levels = rng.integers(0, 5, (TP.BANDS, n)).astype(np.uint8)
            palette = np.stack([T.group_palette(5)] * TP.BANDS)
            yield f"{kind}, {n} tips", reps(lambda: dict(zip(("clear", "bars", "bands", "colour"), eng.plot_tree_raster(
                TP.W, TP.H, lay["panel"], lay["bars"], T.TREE_RGB, levels, palette, lay["bands"], timings=True)[1])))


def run(side, group, lines):
    from ldweaver_amd.engine import Engine
    with Engine(0) as eng, open(lines, "a") as fh:
        for case, ms in globals()["group_" + group](eng):
            fh.write(json.dumps(dict(side=side, group=group, case=case, ms=ms)) + "\n")
            fh.flush()
            print(side, group, case, ms, flush=True)


def merge(lines, out):
    raw = {}
    for rec in map(json.loads, open(lines)):
        for stage, v in rec["ms"].items():
            raw.setdefault(rec["group"], {}).setdefault(rec["case"], {}).setdefault(stage, {}).setdefault(rec["side"], []).extend(v)
    slower = []
    for group, cases in raw.items():
        for case, stages in cases.items():
            for stage, s in stages.items():
                s["branch_median"], s["parent_max"] = float(np.median(s["branch"])), max(s["parent"])
                s["pass"] = s["branch_median"] <= s["parent_max"]
                if not s["pass"]:
                    slower.append(f"{group} / {case} / {stage}")
    with open(out, "w") as fh:
        json.dump(dict(rule="a stage passes when the branch's median is no higher than the parent's largest single value", unit="ms (hip events)",
                       warm_up_calls_per_process=WARM, timed_calls_per_process=REPS, slower=slower, stages=raw), fh, indent=1)
        fh.write("\n")
    print(json.dumps(dict(slower=slower)))
    return 1 if slower else 0


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(*sys.argv[2:5])
    else:
        sys.exit(merge(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "plot_primitives_ab.json")))
