"""The segment map timed on synthetic alignments, beside the per-SNP summary and the LD-decay histogram of the same run.  Needs an MI355X.

    python tools/segment_map_profile.py [OUT.json] [N_SEQS:L_SNPS ...]      (defaults: profiles/segment_map.json, 5000:100000 616:85000)

Per size: the alignment of ldweaver_amd/synth.py made on the device and made resident, its Hamming weights at int(0.1 L) and its SNP meta data set, the
synthetic positions cut into 4 000 equal segments (``segments_equal``); then ``Engine.mi_segment_map`` over ``make_blocks(L, 10000)`` with sr_dist 20 000
and thr 0.1 under the class mask 3 (no distance is computed) and under the mask 2 (circ_len per pair), and ``Engine.mi_segment_best`` under the mask 3 with
the map's own maxima: one warm-up call each, REPS calls timed by the library's own HIP events (``Engine.last_timing()``: the blocks' GEMM + epilogue, the
entry's kernels) and by the host's clock around the call; then ``Engine.mi_snp_summary`` and ``Engine.mi_profile`` the same way (tools/snp_summary_profile.py,
tools/decay_profile.py), whose kernels read the same 8 bytes per pair: the yardsticks.  Recorded:
  * both kernels over the call and per 10^8 pairs, and the bytes they read per second against the rate of a plain device copy measured in the same run;
  * the share of patches on route 2 (``Engine.segment_map_report()``), the values refused and the NaN values;
  * the whole call on the host's clock;
  * k_snp_summary and k_decay_hist over their calls and per 10^8 pairs, and the ratios to them.
No time is required of the run; the file is where the measured numbers go."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "segment_map.json")
SIZES = [tuple(int(v) for v in x.split(":")) for x in sys.argv[2:]] or [(5000, 100000), (616, 85000)]
REPS = 5
BLK = 10000
SR_DIST = 20000.0
THR = 0.1
SEGMENTS = 4000
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from decay_profile import copy_rate                     # noqa: E402
from ldweaver_amd.decay import default_cuts             # noqa: E402
from ldweaver_amd.engine import Engine                  # noqa: E402
from ldweaver_amd.genemap import segments_equal         # noqa: E402
from ldweaver_amd.mi import make_blocks                 # noqa: E402
from ldweaver_amd.snpdat import SnpDat                  # noqa: E402
from ldweaver_amd.synth import synth_alignment          # noqa: E402


def timed(eng, call):
    """One warm-up call, then REPS: (last result, medians of (GEMM + epilogue ms, consumer ms, wall ms), the consumer's min and max)."""
    res = call()
    rows = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        res = call()
        wall = (time.perf_counter() - t0) * 1e3
        t = eng.last_timing()
        rows.append((float(t["gemm_ms"]), float(t["epilogue_ms"]), wall))
    rows = np.asarray(rows)
    return res, [float(v) for v in np.median(rows, axis=0)], float(rows[:, 1].min()), float(rows[:, 1].max())


def main():
    out = {"reps": REPS, "block": BLK, "sr_dist": SR_DIST, "thr": THR, "segments": SEGMENTS, "lib": os.environ.get("LDW_AMD_LIB", ""), "copy_bytes_per_s": copy_rate(),
           "sizes": []}
    rate = out["copy_bytes_per_s"]
    with Engine(0) as eng:
        for N, Ls in SIZES:
            syn = synth_alignment(Ls, N, seed=N, device="cuda")
            eng.set_alignment(syn["states"])
            snp = SnpDat.from_states(None, syn["POS"], float(syn["g"]), counts=eng.state_counts())
            eng.set_weights(eng.hamming_weights(int(0.1 * Ls)))
            eng.set_snp_meta(snp.r, snp.uqe, snp.POS, syn["paint"], snp.g)
            blocks = make_blocks(Ls, BLK)
            seg = segments_equal(snp.POS, int(snp.g), SEGMENTS)
            res, (mi_ms, map_ms, wall_ms), map_min, map_max = timed(eng, lambda: eng.mi_segment_map(blocks, seg, SEGMENTS, SR_DIST, 3, None, THR))
            rep, n = eng.segment_map_report(), int(res["npairs"])
            lres, (_, lr_ms, _), lr_min, lr_max = timed(eng, lambda: eng.mi_segment_map(blocks, seg, SEGMENTS, SR_DIST, 2, None, THR))
            _, (_, best_ms, bwall_ms), best_min, best_max = timed(eng, lambda: eng.mi_segment_best(blocks, seg, SEGMENTS, SR_DIST, 3, res["max"]))
            sres, (_, ss_ms, _), ss_min, ss_max = timed(eng, lambda: eng.mi_snp_summary(blocks, SR_DIST, (THR, THR)))
            dres, (_, dec_ms, _), dec_min, dec_max = timed(eng, lambda: eng.mi_profile(blocks, default_cuts(snp.g), mi_shift=3))
            # (a timing-only ablation build, loaded through LDW_AMD_LIB, counts wrongly on purpose)
            assert out["lib"] or (dres["n_pairs"] == n == int(res["n"].sum()) and int(lres["npairs"]) == int(sres["npairs"][1]))
            n = int(dres["n_pairs"])
            runs = int((np.diff(seg) != 0).sum()) + 1
            row = dict(sequences=N, snps=Ls, blocks=int(len(blocks)), pairs=n, pairs_long_range=int(lres["npairs"]), segment_runs=runs,
                       cells_with_a_pair=int((res["n"] > 0).sum()), blocks_gemm_epilogue_ms=round(mi_ms, 3),
                       segment_map_ms=round(map_ms, 3), segment_map_min_ms=round(map_min, 3), segment_map_max_ms=round(map_max, 3), call_wall_ms=round(wall_ms, 3),
                       segment_map_ms_per_1e8_pairs=round(map_ms * 1e8 / n, 4), segment_map_read_bytes_per_s=8.0 * n / (map_ms * 1e-3),
                       segment_map_read_fraction_of_copy_rate=round(8.0 * n / (map_ms * 1e-3) / rate, 4),
                       segment_map_lr_mask_ms=round(lr_ms, 3), segment_map_lr_mask_min_ms=round(lr_min, 3), segment_map_lr_mask_max_ms=round(lr_max, 3),
                       segment_map_lr_mask_ms_per_1e8_pairs=round(lr_ms * 1e8 / n, 4),
                       segment_best_ms=round(best_ms, 3), segment_best_min_ms=round(best_min, 3), segment_best_max_ms=round(best_max, 3),
                       segment_best_call_wall_ms=round(bwall_ms, 3), segment_best_ms_per_1e8_pairs=round(best_ms * 1e8 / n, 4),
                       segment_best_read_bytes_per_s=8.0 * n / (best_ms * 1e-3), segment_best_read_fraction_of_copy_rate=round(8.0 * n / (best_ms * 1e-3) / rate, 4),
                       patches=rep["patches"], route2_patches=rep["general"], route2_share=round(rep["general"] / max(rep["patches"], 1), 5),
                       values_refused=rep["refused"], nan_values=rep["nan_values"],
                       snp_summary_ms=round(ss_ms, 3), snp_summary_min_ms=round(ss_min, 3), snp_summary_max_ms=round(ss_max, 3),
                       snp_summary_ms_per_1e8_pairs=round(ss_ms * 1e8 / n, 4),
                       decay_hist_ms=round(dec_ms, 3), decay_hist_min_ms=round(dec_min, 3), decay_hist_max_ms=round(dec_max, 3),
                       decay_hist_ms_per_1e8_pairs=round(dec_ms * 1e8 / n, 4),
                       segment_map_over_snp_summary=round(map_ms / ss_ms, 3), segment_map_over_decay_hist=round(map_ms / dec_ms, 3),
                       segment_best_over_snp_summary=round(best_ms / ss_ms, 3))
            out["sizes"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
