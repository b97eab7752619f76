"""The neighbour-joining tree timed on synthetic alignments.  Needs an MI355X.

    python tools/nj_profile.py [OUT.json] [L_SNPS] [N_SEQS ...]      (defaults: profiles/nj_tree.json, 20000, 616 5000 10000)

Per size: the alignment of ldweaver_amd/synth.py made resident, one warm-up call of ``Engine.nj_tree()``, then REPS calls timed by the library's own
HIP events (``Engine.last_timing()``: the joins alone, and the Hamming GEMM + the fill of d and r in front of them) and by the host's clock around
the call.  The joins read the active n x n matrix once each: sum of 8 n^2 bytes over the joins, divided by their time, against the rate of a plain
device copy (``torch`` ``copy_`` of 1 GiB, read + written bytes per second) measured in the same run.  No time is required of the run; the file is
where the measured numbers go.

    python tools/nj_profile.py --bootstrap [OUT.json] [L_SNPS] [N_SEQS ...]      (defaults: profiles/nj_bootstrap.json, 20000, 616 5000)

The bootstrap mode: per size, the single tree as above (one warm-up, three calls: the yardstick of the same run), then ``Engine.nj_bootstrap`` of
B = 32 replicates drawn by ``bootstrap_multiplicities`` with LDW_NJ_BATCH=1, with LDW_NJ_BATCH=4 and with the library's own batch size, alternating,
one warm-up and three calls each, their results compared byte for byte; from the library's events, per replicate: digits + GEMM + fill, joins, split sums + look-ups."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOOTSTRAP = len(sys.argv) > 1 and sys.argv[1] == "--bootstrap"
if BOOTSTRAP:
    del sys.argv[1]
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "nj_bootstrap.json" if BOOTSTRAP else "nj_tree.json")
L_SNPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
SIZES = [int(x) for x in sys.argv[3:]] or ([616, 5000] if BOOTSTRAP else [616, 5000, 10000])
REPS = 5
BOOT_B, BOOT_REPS = 32, 3
sys.path.insert(0, ROOT)
from ldweaver_amd.engine import Engine                 # noqa: E402
from ldweaver_amd.synth import synth_alignment         # noqa: E402
import torch                                           # noqa: E402


def copy_rate() -> float:
    """Bytes read + written per second by a device-to-device copy of 1 GiB (the best of 5 after a warm-up)."""
    a = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    b.copy_(a)
    best = float("inf")
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    del a, b
    torch.cuda.empty_cache()
    return 2.0 * (1 << 30) / (best * 1e-3)


def bootstrap_profile():
    from ldweaver_amd.tree import bootstrap_multiplicities
    out = {"snps": L_SNPS, "replicates": BOOT_B, "reps": BOOT_REPS, "sizes": []}
    med = lambda xs: round(float(np.median(xs)), 4)     # noqa: E731
    with Engine(0) as eng:
        for N in SIZES:
            eng.set_alignment(np.ascontiguousarray(synth_alignment(L_SNPS, N, seed=N)["states"]))
            mult = bootstrap_multiplicities(L_SNPS, BOOT_B, seed=N)
            eng.nj_tree()
            single = []
            for _ in range(BOOT_REPS):
                eng.nj_tree()
                single.append(float(eng.last_timing()["gemm_ms"]))
            modes = {"batch_1": "1", "batch_4": "4", "batch_default": None}
            got = {k: dict(prep=[], joins=[], hash=[], wall=[]) for k in modes}
            results = {}
            for rep in range(BOOT_REPS + 1):            # (the first round warms both)
                for tag, value in modes.items():
                    os.environ.pop("LDW_NJ_BATCH", None)
                    if value is not None:
                        os.environ["LDW_NJ_BATCH"] = value
                    t0 = time.perf_counter()
                    res = eng.nj_bootstrap(mult)
                    wall = (time.perf_counter() - t0) * 1e3
                    results.setdefault(tag, res)
                    assert all(a.tobytes() == b.tobytes() for a, b in zip(res, results["batch_1"]))
                    if rep:
                        t = eng.last_timing()
                        for k, v in (("prep", t["epilogue_ms"]), ("joins", t["gemm_ms"]), ("hash", t["select_ms"]), ("wall", wall)):
                            got[tag][k].append(float(v) / BOOT_B)
            os.environ.pop("LDW_NJ_BATCH", None)
            row = dict(sequences=N, single_tree_joins_ms=med(single), min_support=int(results["batch_1"][2][N:2 * N - 3].min()),
                       max_support=int(results["batch_1"][2][N:2 * N - 3].max()))
            for tag in modes:
                g = got[tag]
                row[tag] = dict(ms_per_replicate=med([a + b + c for a, b, c in zip(g["prep"], g["joins"], g["hash"])]), digits_gemm_fill_ms=med(g["prep"]),
                                joins_ms=med(g["joins"]), joins_min_ms=round(min(g["joins"]), 4), joins_max_ms=round(max(g["joins"]), 4),
                                sums_lookup_ms=med(g["hash"]), call_wall_ms_per_replicate=med(g["wall"]))
            out["sizes"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if BOOTSTRAP:
    bootstrap_profile()
    sys.exit(0)

out = {"snps": L_SNPS, "reps": REPS, "copy_bytes_per_s": copy_rate(), "sizes": []}
with Engine(0) as eng:
    for N in SIZES:
        states = np.ascontiguousarray(synth_alignment(L_SNPS, N, seed=N)["states"])
        eng.set_alignment(states)
        parent, _ = eng.nj_tree()                      # warm: code objects, the device blocks of the pool
        assert parent[2 * N - 3] == -1 and int((parent == 2 * N - 3).sum()) == 3
        joins, init, wall = [], [], []
        for _ in range(REPS):
            t0 = time.perf_counter()
            eng.nj_tree()
            wall.append((time.perf_counter() - t0) * 1e3)
            t = eng.last_timing()
            joins.append(float(t["gemm_ms"]))
            init.append(float(t["epilogue_ms"]))
            per_join = float(t["select_ms"])
        scanned = float(sum(8 * n * n for n in range(4, N + 1)))
        med = float(np.median(joins))
        row = dict(sequences=N, joins=N - 3, launches_per_join=per_join, joins_ms=dict(median=round(med, 3), min=round(min(joins), 3), max=round(max(joins), 3)),
                   init_ms=round(float(np.median(init)), 3), call_wall_ms=round(float(np.median(wall)), 3), us_per_join=round(med * 1e3 / (N - 3), 3),
                   scanned_bytes=scanned, scan_bytes_per_s=round(scanned / (med * 1e-3), 1),
                   fraction_of_copy_rate=round(scanned / (med * 1e-3) / out["copy_bytes_per_s"], 4))
        out["sizes"].append(row)
        print(json.dumps(row), flush=True)
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
