"""Times of the gene-network step on an annotated link file written by the library's own writer: create_network_for_gene at level 1 and
at level 2 (about 100 neighbour genes), native against pandas on the same file, the search's rate beside ldw_tsv_read's on a numeric file of the same
byte size, and the capsule renderer on the default canvas.  Needs an MI355X.

    python tools/network_profile.py [OUT.json] [SCRATCH_DIR] [ROWS]      (defaults: profiles/network_grep.json, a temporary directory, 1e7)

The driver runs every step as a child process under a time limit of its own and stops at the first one that fails; a step writes its numbers to
SCRATCH_DIR/<step>.json and the driver merges them.  2 warm-up calls, then the median of 3; host wall time round calls that synchronise before they return."""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = (("make", 900), ("native", 600), ("pandas", 1100), ("yardstick", 600), ("render", 300))     # name, seconds
GENES = 120


def timed(fn, warm=2, reps=3):
    v = []
    for rep in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        if rep >= warm:
            v.append(time.perf_counter() - t0)
    return float(np.median(v)), [round(x, 4) for x in v]


def paths(tmp):
    return os.path.join(tmp, "sr_links_annotated.tsv"), os.path.join(tmp, "numeric.tsv")


def step_make(tmp, n):
    """The annotated file through annotate.write_links_table, and a numeric table of (about) the same byte size through write_table_tsv."""
    from ldweaver_amd import _lib as L
    from ldweaver_amd import annotate as A
    from ldweaver_amd.engine import write_table_tsv
    rng = np.random.default_rng(3)
    snps = 50_000
    gene_of = rng.integers(0, 2000, snps)
    table = [f"gene{gene_of[k]:04d}:{k}:missense_variant:p.Ala{k % 400}Val" for k in range(snps)] + [f"gene{gene_of[k]:04d}_region" for k in range(snps)] + \
            [f"A:{(k % 97) / 97:.3f}" for k in range(snps)] + ["syXsy", "nsXsy", "syXns", "nsXns"]
    # gene0000 is linked three times or more to about GENES genes: the level-2 needles
    r1, r2 = rng.integers(0, snps, n).astype(np.int32), rng.integers(0, snps, n).astype(np.int32)
    of0 = np.nonzero(gene_of == 0)[0]
    hubs = rng.choice(np.arange(1, 2000), GENES, replace=False)
    for h in hubs:
        to = np.nonzero(gene_of == h)[0]
        at = rng.integers(0, n, 4)
        r1[at], r2[at] = rng.choice(of0, 4), rng.choice(to, 4)
    pos1 = rng.integers(1, 2_000_000, n).astype(np.int64)
    num = [("pos1", L.COL_INT64, pos1), ("pos2", L.COL_INT64, pos1 + rng.integers(1, 20000, n)), ("len", L.COL_DOUBLE, rng.integers(1, 20000, n).astype(np.float64)),
           ("ARACNE", L.COL_DOUBLE, (rng.random(n) < 0.7).astype(np.float64)), ("MI", L.COL_DOUBLE, rng.random(n) ** 3), ("srp", L.COL_DOUBLE, rng.random(n) * 9)]
    strs = [("pos1_ann", 0, r1), ("pos2_ann", 0, r2), ("pos1_genreg", snps, r1), ("pos2_genreg", snps, r2), ("pos1_ad", 2 * snps, r1), ("pos2_ad", 2 * snps, r2),
            ("links", 3 * snps, rng.integers(0, 4, n).astype(np.int32))]
    ann, numeric = paths(tmp)
    A.write_links_table(ann, A.SR_COLS, num, strs, table)
    size = os.path.getsize(ann)
    x = np.floor(rng.random(n) * 50000.0) + 1.0
    rows = n
    while True:      # nine numeric columns, rows scaled until the sizes agree within 2 %
        cols = [(np.arange(rows) % 3 + 1).astype(np.int32), np.resize(x, rows).astype(np.int32), np.resize(x + 17, rows).astype(np.int32)] + \
               [np.resize(rng.random(n), rows) for _ in range(6)]
        write_table_tsv(numeric, cols, append=False)
        got = os.path.getsize(numeric)
        if abs(got - size) <= 0.02 * size:
            break
        rows = int(rows * size / got)
    return dict(rows=n, annotated_bytes=size, numeric_bytes=got, numeric_rows=rows, neighbour_genes_planted=GENES)


def step_native(tmp, n):
    from ldweaver_amd import network as N
    from ldweaver_amd.engine import Engine
    ann, _ = paths(tmp)
    out = {}
    with Engine(0) as eng:
        for level in (1, 2):
            stats, frames = [], []

            def run():
                frames.append(N.create_network_for_gene("gene0000", ann, level=level, engine=eng))
                stats.append(eng.links_grep_stats())
            med, allv = timed(run)
            st = {k: float(np.median([s[k] for s in stats[2:]])) for k in ("total_ms", "read_ms", "copy_ms", "line_ms", "grep_ms")}
            st.update(s=med, all_s=allv, rows_returned=len(frames[-1]), chunks=stats[-1]["chunks"], bytes=stats[-1]["bytes"],
                      search_GBps=stats[-1]["bytes"] / (st["total_ms"] * 1e-3) / 1e9, kernel_share=st["grep_ms"] / st["total_ms"], read_share=st["read_ms"] / st["total_ms"])
            out[f"native_level{level}"] = st
            frames[-1].to_pickle(os.path.join(tmp, f"native_level{level}.pkl"))
    return out


def step_pandas(tmp, n):
    import pandas as pd
    from ldweaver_amd import network as N
    ann, _ = paths(tmp)
    out = {}
    for level in (1, 2):
        frames = []
        med, allv = timed(lambda: frames.append(N.create_network_for_gene("gene0000", ann, level=level, reader="pandas")))
        out[f"pandas_level{level}"] = dict(s=med, all_s=allv, rows_returned=len(frames[-1]))
        out[f"identical_level{level}"] = bool(frames[-1].equals(pd.read_pickle(os.path.join(tmp, f"native_level{level}.pkl"))))
    return out


def step_yardstick(tmp, n):
    from ldweaver_amd.engine import Engine
    _, numeric = paths(tmp)
    with Engine(0) as eng:
        stats = []

        def run():
            eng.tsv_read(numeric, "\t", 9)
            stats.append(eng.tsv_stats())
        med, allv = timed(run)
    return dict(tsv_read_s=med, tsv_read_all_s=allv, tsv_read_GBps=stats[-1]["bytes"] / med / 1e9)


def step_render(tmp, n):
    import pandas as pd
    from ldweaver_amd import network as N
    from ldweaver_amd.engine import Engine
    rng = np.random.default_rng(1)
    k = 1000
    a = rng.integers(0, 400, k)
    b = (a + 1 + rng.integers(0, 398, k)) % 400
    e = pd.DataFrame({"p1": [f"g{i}" for i in a], "p2": [f"g{i}" for i in b], "Num_Links": rng.integers(2, 9, k), "weights": rng.random(k)})
    names, xy, _ = N.network_layout(e, 6000, 4000)
    caps, _, _ = N.network_capsules(e, names, xy, 6000)
    with Engine(0) as eng:
        ms = [eng.plot_capsules(caps, 6000, 4000, timings=True)[1] for _ in range(5)][2:]
    return dict(render_edges=k, render_capsules=len(caps), binning_ms=float(np.median([m[0] for m in ms])), shading_ms=float(np.median([m[1] for m in ms])))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        name, tmp, n = sys.argv[2], sys.argv[3], int(sys.argv[4])
        res = globals()["step_" + name](tmp, n)
        with open(os.path.join(tmp, name + ".json"), "w") as f:
            json.dump(res, f)
        print(json.dumps(res), flush=True)
        return 0
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "network_grep.json")
    tmp = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="ldw_net_")
    n = int(float(sys.argv[3])) if len(sys.argv) > 3 else 10_000_000
    os.makedirs(tmp, exist_ok=True)
    out = {"warm_up_calls": 2, "timed_calls": 3}
    for name, limit in STEPS:
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, tmp, str(n)]).returncode
        if rc != 0:
            print(f"step {name} ended with status {rc}: stopping", file=sys.stderr)
            return rc
        with open(os.path.join(tmp, name + ".json")) as f:
            out.update(json.load(f))
    for level in (1, 2):
        out[f"native_over_pandas_level{level}"] = out[f"native_level{level}"]["s"] / out[f"pandas_level{level}"]["s"]
    out["native_not_slower"] = all(out[f"native_over_pandas_level{k}"] <= 1.0 for k in (1, 2))
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
    for p in paths(tmp):
        os.remove(p)
    return 0 if out["native_not_slower"] and out["identical_level1"] and out["identical_level2"] else 1


if __name__ == "__main__":
    sys.exit(main())
