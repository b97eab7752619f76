"""Times of the tree view: for a random binary tree and for a caterpillar of 1e3, 1e4 and 7e4 tips with 40 allele bands on the default
canvas (4500 x 6000), the hip-event times of the renderer's four stages (clear, bars, bands, colour: ldw_debug_plot_tree) and the host times of parse,
midpoint rooting, ladderize and layout; and the caterpillar-to-random ratio of the bars stage.  Needs an MI355X.

    python tools/tree_profile.py [OUT.json]      (default: profiles/tree_render.json)

Every case runs in a child process under a time limit of its own; the driver stops at the first that fails.  2 warm-up renders, then the median of 5."""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (1000, 10000, 70000)
KINDS = ("random", "caterpillar")
BANDS, W, H = 40, 4500, 6000
LIMIT = 300     # seconds per case


def newick(kind, n, rng):
    if kind == "caterpillar":
        return ("(" * (n - 1) + "t0:1" + "".join(f",t{k}:{1 + k % 3}):1" for k in range(1, n)))[:-2] + ";"
    items = [f"t{k}:{float(rng.random()) + 0.01:.4f}" for k in range(n)]
    while len(items) > 1:      # random joins of two subtrees
        i, j = sorted(rng.choice(len(items), 2, replace=False).tolist())
        b, a = items.pop(j), items.pop(i)
        items.append(f"({a},{b})" + (f":{float(rng.random()) + 0.01:.4f}" if items else ""))
    return items[0] + ";"


def case(kind, n, out_path):
    from ldweaver_amd import tree as T
    from ldweaver_amd.engine import Engine
    rng = np.random.default_rng(n)
    text = newick(kind, n, rng).encode()
    host = {}

    def clock(name, fn):
        t0 = time.perf_counter()
        r = fn()
        host[name + "_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
        return r

    tree = clock("parse", lambda: T.parse_newick(text))
    tree = clock("root", lambda: T.midpoint_root(tree))
    tree = clock("ladderize", lambda: T.ladderize(tree))
    lay = clock("layout", lambda: T.tree_layout(tree, W, H, 0, BANDS, band_labels=["1234567"] * BANDS, legends=[("Metadata", [], []), ("Alleles", list("ACGTN"), [0] * 5)]))
    levels = rng.integers(0, 5, (BANDS, n)).astype(np.uint8)
    palette = np.stack([T.group_palette(5)] * BANDS)
    eng = Engine(0)
    try:
        ms = []
        for rep in range(7):
            _, t = eng.plot_tree_raster(W, H, lay["panel"], lay["bars"], T.TREE_RGB, levels, palette, lay["bands"], timings=True)
            if rep >= 2:
                ms.append(t)
    finally:
        eng.close()
    med = np.median(np.asarray(ms), axis=0)
    with open(out_path, "w") as fh:
        json.dump(dict(kind=kind, tips=n, bars=int(len(lay["bars"])), panel=[int(v) for v in lay["panel"]], clear_ms=round(float(med[0]), 4), bars_ms=round(float(med[1]), 4),
                       bands_ms=round(float(med[2]), 4), colour_ms=round(float(med[3]), 4), **host), fh)


def main():
    if len(sys.argv) >= 5 and sys.argv[1] == "--case":
        return case(sys.argv[2], int(sys.argv[3]), sys.argv[4])
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tree_render.json")
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for n in SIZES:
            for kind in KINDS:
                part = os.path.join(tmp, f"{kind}_{n}.json")
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", kind, str(n), part], timeout=LIMIT)
                if r.returncode != 0:
                    sys.exit(f"tree_profile: the case {kind} {n} ended with status {r.returncode}; nothing written")
                rows.append(json.load(open(part)))
                print(rows[-1], flush=True)
    ratio = {str(n): round(next(r["bars_ms"] for r in rows if r["tips"] == n and r["kind"] == "caterpillar") /
                           max(next(r["bars_ms"] for r in rows if r["tips"] == n and r["kind"] == "random"), 1e-9), 2) for n in SIZES}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(dict(canvas=[W, H], bands=BANDS, cases=rows, bars_caterpillar_over_random=ratio), fh, indent=1)
    print(json.dumps(dict(bars_caterpillar_over_random=ratio)))


if __name__ == "__main__":
    main()
