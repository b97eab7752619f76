"""The per-SNP MI summary timed on synthetic alignments, beside the LD-decay histogram of the same run.  Needs an MI355X.

    python tools/snp_summary_profile.py [OUT.json] [N_SEQS:L_SNPS ...]      (defaults: profiles/snp_summary.json, 5000:100000 616:85000)

Per size: the alignment of ldweaver_amd/synth.py made on the device and made resident, its Hamming weights at int(0.1 L) and its SNP meta data set, then
``Engine.mi_snp_summary`` over ``make_blocks(L, 10000)`` with sr_dist 20 000 and the thresholds (0.1, 0.1): one warm-up call, REPS calls timed by the
library's own HIP events (``Engine.last_timing()``: the blocks' GEMM + epilogue, the summary kernels) and by the host's clock around the call; then
``Engine.mi_profile`` the same way (tools/decay_profile.py), whose kernel reads the same 8 bytes per pair: the yardstick.  Recorded:
  * k_snp_summary over the call and per 10^8 pairs, and the bytes it reads per second against the rate of a plain device copy measured in the same run;
  * the share of its patches on the general route (``Engine.snp_summary_report()``), the pairs off their patch's class and the values refused;
  * the whole call on the host's clock;
  * k_decay_hist over its call and per 10^8 pairs, and the ratio of the two kernels.
No time is required of the run; the file is where the measured numbers go."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "snp_summary.json")
SIZES = [tuple(int(v) for v in x.split(":")) for x in sys.argv[2:]] or [(5000, 100000), (616, 85000)]
REPS = 5
BLK = 10000
SR_DIST = 20000.0
THR = (0.1, 0.1)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from decay_profile import copy_rate                     # noqa: E402
from ldweaver_amd.background import exact_sum        # noqa: E402
from ldweaver_amd.decay import default_cuts             # noqa: E402
from ldweaver_amd.engine import Engine                  # noqa: E402
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
    out = {"reps": REPS, "block": BLK, "sr_dist": SR_DIST, "thr": list(THR), "lib": os.environ.get("LDW_AMD_LIB", ""), "copy_bytes_per_s": copy_rate(),
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
            res, (mi_ms, ss_ms, wall_ms), ss_min, ss_max = timed(eng, lambda: eng.mi_snp_summary(blocks, SR_DIST, THR))
            rep, n = eng.snp_summary_report(), int(res["npairs"].sum())
            dres, (dmi_ms, dec_ms, dwall_ms), dec_min, dec_max = timed(eng, lambda: eng.mi_profile(blocks, default_cuts(snp.g), mi_shift=3))
            # (a timing-only ablation build, loaded through LDW_AMD_LIB, counts wrongly on purpose)
            assert out["lib"] or (dres["n_pairs"] == n and np.array_equal(res["n"].sum(axis=1), 2 * res["npairs"]))
            n = int(dres["n_pairs"])
            read_rate = 8.0 * n / (ss_ms * 1e-3)
            row = dict(sequences=N, snps=Ls, blocks=int(len(blocks)), pairs=n, pairs_short_range=int(res["npairs"][0]),
                       blocks_gemm_epilogue_ms=round(mi_ms, 3), snp_summary_ms=round(ss_ms, 3), snp_summary_min_ms=round(ss_min, 3),
                       snp_summary_max_ms=round(ss_max, 3), call_wall_ms=round(wall_ms, 3), snp_summary_ms_per_1e8_pairs=round(ss_ms * 1e8 / n, 4),
                       snp_summary_read_bytes_per_s=read_rate, snp_summary_read_fraction_of_copy_rate=round(read_rate / rate, 4),
                       patches=rep["patches"], general_route_patches=rep["general"], general_route_share=round(rep["general"] / max(rep["patches"], 1), 5),
                       pairs_off_their_patch_class=rep["off_class"], values_refused=rep["refused"],
                       decay_hist_ms=round(dec_ms, 3), decay_hist_min_ms=round(dec_min, 3), decay_hist_max_ms=round(dec_max, 3),
                       decay_hist_ms_per_1e8_pairs=round(dec_ms * 1e8 / n, 4), decay_call_wall_ms=round(dwall_ms, 3),
                       snp_summary_over_decay_hist=round(ss_ms / dec_ms, 3), overall_mean_lr=float(exact_sum(res["sumq"][1]) / max(exact_sum(res["n"][1]), 1) / 2.0 ** 40))
            out["sizes"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
