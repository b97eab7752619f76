"""The co-change scan timed on synthetic alignments, on the device's own neighbour-joining tree.  Needs an MI355X.

    python tools/cochange_scan_profile.py [OUT.json] [N_SEQS:L_SNPS ...]      (defaults: profiles/cochange_scan.json, 5000:100000 616:85000)

Per size: the alignment of ldweaver_amd/synth.py made resident, ``Engine.nj_tree()`` and ``tree_from_joins`` for the tree; then, for min_changes 1 and 2,
``Engine.tree_cochange_scan`` and ``Engine.tree_cochange_links`` (at ``pick_min_co(hist, TOP)``, the exact capacity, the scan's bests): one warm-up call,
REPS calls timed by the library's own HIP events (``Engine.last_timing()``: the pair kernels, the parsimony passes with their gathers, the copies out;
medians) and by the host's clock around the call.  Recorded with them: M (the eligible SNPs), the pairs of the pair set, and the lane-operations per second
of the pair kernel against the arithmetic floor of the section — pairs x words x 2 (one AND, one counting add per pair and 32-bit word); the floor is a
derivation, the rate is the measurement.
For comparison the only other route to the same integers, ``Engine.tree_cochanges`` on a listed sample of SAMPLE of the same pairs: its pair kernel's time
(with the copies behind it) per pair, scaled to all pairs of the set and labelled as scaled; the sample's co is checked against the links the scan listed.
No time is required of the run; the file is where the measured numbers go."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "cochange_scan.json")
SIZES = [tuple(int(v) for v in x.split(":")) for x in sys.argv[2:]] or [(5000, 100000), (616, 85000)]
REPS = 5
TOP = 1000
SAMPLE = 1000000
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pars_ref                                        # noqa: E402
from ldweaver_amd.engine import Engine                 # noqa: E402
from ldweaver_amd.parsimony import pick_min_co         # noqa: E402
from ldweaver_amd.synth import synth_alignment         # noqa: E402
from ldweaver_amd.tree import tree_from_joins          # noqa: E402


def timed(eng, call):
    """One warm-up, then REPS calls: (the last result, medians of the three event times and of the host's clock in ms, min and max of the pair kernels)."""
    call()
    rows, res = [], None
    for _ in range(REPS):
        t0 = time.perf_counter()
        res = call()
        wall = (time.perf_counter() - t0) * 1e3
        t = eng.last_timing()
        rows.append((float(t["gemm_ms"]), float(t["epilogue_ms"]), float(t["select_ms"]), wall))
    r = np.asarray(rows)
    return res, np.median(r, axis=0), float(r[:, 0].min()), float(r[:, 0].max())


def main():
    out = {"reps": REPS, "top": TOP, "sample": SAMPLE, "lib": os.environ.get("LDW_AMD_LIB", ""), "runs": []}
    rng = np.random.default_rng(1)
    with Engine(0) as eng:
        for N, Ls in SIZES:
            states = np.ascontiguousarray(synth_alignment(Ls, N, seed=N)["states"])
            eng.set_alignment(states)
            par, ln = eng.nj_tree()
            parent, tip_seq = pars_ref.from_tree(tree_from_joins(par, ln))
            nodes = len(parent)
            words = (nodes + 31) // 32
            for min_changes in (1, 2):
                kw = dict(gap_mode=0, min_changes=min_changes, min_lift=0, min_len=-1.0)
                scan, sm, s_lo, s_hi = timed(eng, lambda: eng.tree_cochange_scan(parent, tip_seq, min_co=2, **kw))
                M, pairs = int((scan["changes"] >= min_changes).sum()), scan["npairs"]
                assert pairs == M * (M - 1) // 2 and int(scan["hist"].sum()) == scan["n_qualifying"] == pairs
                min_co = pick_min_co(scan["hist"], TOP)
                cap = eng.tree_cochange_links(parent, tip_seq, min_co=min_co, cap=0, **kw)["count"]
                lk, lm, l_lo, l_hi = timed(eng, lambda: eng.tree_cochange_links(parent, tip_seq, min_co=min_co, cap=cap, best_in=scan["best"], **kw))
                assert lk["count"] == cap == int(scan["hist"][min_co:].sum()) or min_co == 1023
                floor_ops = float(pairs) * words * 2.0
                row = dict(sequences=N, snps=Ls, nodes=nodes, words=words, min_changes=min_changes, eligible_snps=M, pairs=pairs,
                           scan_pair_kernel_ms=round(float(sm[0]), 3), scan_pair_kernel_min_ms=round(s_lo, 3), scan_pair_kernel_max_ms=round(s_hi, 3),
                           scan_passes_ms=round(float(sm[1]), 3), scan_copies_ms=round(float(sm[2]), 3), scan_call_wall_ms=round(float(sm[3]), 3),
                           links_pair_kernel_ms=round(float(lm[0]), 3), links_pair_kernel_min_ms=round(l_lo, 3), links_pair_kernel_max_ms=round(l_hi, 3),
                           links_passes_ms=round(float(lm[1]), 3), links_copies_ms=round(float(lm[2]), 3), links_call_wall_ms=round(float(lm[3]), 3),
                           min_co=min_co, listed=cap, floor_lane_ops=floor_ops, scan_lane_ops_per_s=floor_ops / (float(sm[0]) * 1e-3),
                           links_lane_ops_per_s=floor_ops / (float(lm[0]) * 1e-3), best_co_max=int(scan["best"].max()))
                # the listed route on a sample of the same pairs
                idx = np.flatnonzero(scan["changes"] >= min_changes).astype(np.int32)
                K = int(min(SAMPLE, pairs))
                a, b = idx[rng.integers(0, M, size=K)], idx[rng.integers(0, M, size=K)]
                if cap:                                    # (the listed pairs among them: their co is known)
                    a[:min(cap, K)], b[:min(cap, K)] = lk["a"][:K], lk["b"][:K]
                rows = []
                eng.tree_cochanges(parent, tip_seq, a, b, 0)
                for _ in range(REPS):
                    ca, cb, co = eng.tree_cochanges(parent, tip_seq, a, b, 0)
                    t = eng.last_timing()
                    rows.append((float(t["select_ms"]), float(t["gemm_ms"]) + float(t["epilogue_ms"])))
                assert not cap or np.array_equal(co[:min(cap, K)], lk["co"][:K])
                pm = np.median(np.asarray(rows), axis=0)
                row.update(listed_route_pairs=K, listed_route_pair_kernel_and_copies_ms=round(float(pm[0]), 3), listed_route_passes_ms=round(float(pm[1]), 3),
                           listed_route_pair_ms_scaled_to_all_pairs=round(float(pm[0]) / K * pairs, 1))
                out["runs"].append(row)
                print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
