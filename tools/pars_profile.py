"""Parsimony on a tree timed on synthetic alignments, on the device's own neighbour-joining tree.  Needs an MI355X.

    python tools/pars_profile.py [OUT.json] [N_SEQS:L_SNPS ...]      (defaults: profiles/parsimony.json, 5000:100000 616:85000)

Per size: the alignment of ldweaver_amd/synth.py made resident, ``Engine.nj_tree()`` and ``tree_from_joins`` for the tree, then
  * ``Engine.tree_parsimony`` (all SNPs): one warm-up call, REPS calls timed by the library's own HIP events (``Engine.last_timing()``: the gathers of the
    tips' states, the up passes) and by the host's clock around the call;
  * ``Engine.tree_cochanges`` for 250 and for 10^6 random pairs, the same way (gathers, up + down passes, the pair kernel with what follows);
  * the numpy restatement (tests/pars_ref.py ``up_pass``) on the first REF_COLS columns of the same alignment and tree, on the host's clock, and that
    time scaled to all columns (its loop over the nodes is vectorised over the columns: the scaling is an extrapolation and is marked as one).
The bytes a pass moves are counted from the statement — the gather reads and writes tips x L, the up pass reads every child's set once and writes every
set of a node with children, the down pass reads a node's and its parent's and writes the node's — and set against the rate of a plain device copy
(``torch`` ``copy_`` of 1 GiB, read + written bytes per second) measured in the same run.  No time is required of the run; the file is where the measured
numbers go."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "parsimony.json")
SIZES = [tuple(int(v) for v in x.split(":")) for x in sys.argv[2:]] or [(5000, 100000), (616, 85000)]
REPS = 5
REF_COLS = 2000
PAIR_COUNTS = (250, 1000000)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pars_ref                                        # noqa: E402
from ldweaver_amd.engine import Engine                 # noqa: E402
from ldweaver_amd.synth import synth_alignment         # noqa: E402
from ldweaver_amd.tree import tree_from_joins          # noqa: E402
import torch                                           # noqa: E402


def copy_rate() -> float:
    """Bytes read + written per second by a device-to-device copy of 1 GiB (the best of 5 after a warm-up), as tools/nj_profile.py measures it."""
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


def timed(eng, call):
    """One warm-up, then REPS calls: medians of the library's three event times and of the host's clock, in ms."""
    call()
    rows = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        wall = (time.perf_counter() - t0) * 1e3
        t = eng.last_timing()
        rows.append((float(t["epilogue_ms"]), float(t["gemm_ms"]), float(t["select_ms"]), wall))
    m = np.median(np.asarray(rows), axis=0)
    lo = np.min(np.asarray(rows), axis=0)
    hi = np.max(np.asarray(rows), axis=0)
    return dict(gather_ms=round(float(m[0]), 3), passes_ms=round(float(m[1]), 3), passes_min_ms=round(float(lo[1]), 3), passes_max_ms=round(float(hi[1]), 3),
                after_ms=round(float(m[2]), 3), call_wall_ms=round(float(m[3]), 3))


out = {"reps": REPS, "copy_bytes_per_s": copy_rate(), "sizes": []}
rng = np.random.default_rng(1)
with Engine(0) as eng:
    for N, Ls in SIZES:
        states = np.ascontiguousarray(synth_alignment(Ls, N, seed=N)["states"])
        eng.set_alignment(states)
        t0 = time.perf_counter()
        par, ln = eng.nj_tree()
        nj_ms = (time.perf_counter() - t0) * 1e3
        parent, tip_seq = pars_ref.from_tree(tree_from_joins(par, ln))
        nodes, inner = len(parent), len(parent) - N
        row = dict(sequences=N, snps=Ls, nodes=nodes, nj_tree_wall_ms=round(nj_ms, 1))
        # all-SNP scoring
        sc = timed(eng, lambda: eng.tree_parsimony(parent, tip_seq, 0))
        gather_bytes, up_bytes = 2.0 * N * Ls, float(nodes - 1 + inner) * Ls
        sc.update(gather_bytes=gather_bytes, up_bytes=up_bytes, gather_fraction_of_copy_rate=round(gather_bytes / (sc["gather_ms"] * 1e-3) / out["copy_bytes_per_s"], 4),
                  up_fraction_of_copy_rate=round(up_bytes / (sc["passes_ms"] * 1e-3) / out["copy_bytes_per_s"], 4), ns_per_node=round(sc["passes_ms"] * 1e6 / nodes, 1))
        row["scoring"] = sc
        score, _ = eng.tree_parsimony(parent, tip_seq, 0)
        # the numpy restatement on the first REF_COLS columns
        cols = min(REF_COLS, Ls)
        sub = np.ascontiguousarray(states[:cols])
        t0 = time.perf_counter()
        _, ref_score = pars_ref.up_pass(parent, tip_seq, sub, 0)
        ref_s = time.perf_counter() - t0
        assert np.array_equal(ref_score, score[:cols])
        row["numpy_reference"] = dict(columns=cols, seconds=round(ref_s, 2), seconds_scaled_to_all_columns_extrapolated=round(ref_s * Ls / cols, 1))
        # co-changes
        for K in PAIR_COUNTS:
            a, b = rng.integers(0, Ls, size=K).astype(np.int32), rng.integers(0, Ls, size=K).astype(np.int32)
            distinct = int(len(np.unique(np.concatenate([a, b]))))
            co = timed(eng, lambda: eng.tree_cochanges(parent, tip_seq, a, b, 0))
            ca, cb, cc = eng.tree_cochanges(parent, tip_seq, a, b, 0)
            assert np.array_equal(ca, score[a]) and np.array_equal(cb, score[b]) and np.all(cc <= np.minimum(ca, cb))
            pass_bytes = (float(nodes - 1 + inner) + 3.0 * (nodes - 1)) * distinct
            co.update(pairs=K, distinct_snps=distinct, up_down_bytes=pass_bytes,
                      up_down_fraction_of_copy_rate=round(pass_bytes / (co["passes_ms"] * 1e-3) / out["copy_bytes_per_s"], 4),
                      pair_bitmap_bytes=2.0 * 4 * ((nodes + 31) // 32) * K)
            row[f"cochanges_{K}"] = co
        out["sizes"].append(row)
        print(json.dumps(row), flush=True)
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
