"""Selection by the corrected score timed on synthetic alignments, beside the LD-decay histogram and the per-SNP summary of the same run.
Needs an MI355X.

    python tools/score_select_profile.py [OUT.json] [N_SEQS:L_SNPS ...]      (defaults: profiles/score_select.json, 5000:100000 616:85000)

Per size: the alignment of ldweaver_amd/synth.py made on the device and made resident, its Hamming weights at int(0.1 L) and its SNP meta data set; blocks
``make_blocks(L, 10000)``, sr_dist 20 000.  Each of the four walks is called once to warm up, then REPS times, timed by the library's own HIP events
(``Engine.last_timing()``: the blocks' GEMM + epilogue, the consumer's kernels; medians) and by the host's clock around the call:
  * ``Engine.mi_snp_summary`` (k_snp_summary) and ``Engine.mi_profile`` (k_decay_hist): the yardsticks, unchanged kernels reading the same 8 bytes per pair;
  * ``Engine.mi_score_scan`` (k_score_scan) with the long-range mask and the weights of the average product correction from that summary;
  * ``Engine.mi_score_links`` (k_score_links) with ``pick_threshold(hist, 1000)`` and the scan's bests.
Recorded besides: the two ratios the issue names (links / summary, scan / (histogram + summary)), the share of pairs with a score in bucket 0, the bytes
each kernel reads per second against the rate of a plain device copy measured in the same run, and ``apc_links``' whole call (scan, threshold, links, sort)
on the host's clock with the background given and the alignment resident.  No time is required of the run; the file is where the measured numbers go."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "score_select.json")
SIZES = [tuple(int(v) for v in x.split(":")) for x in sys.argv[2:]] or [(5000, 100000), (616, 85000)]
REPS = 5
BLK = 10000
SR_DIST = 20000.0
TOP = 1000
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from decay_profile import copy_rate                     # noqa: E402
from snp_summary_profile import timed                   # noqa: E402
from ldweaver_amd import background as B                # noqa: E402
from ldweaver_amd.decay import default_cuts             # noqa: E402
from ldweaver_amd.engine import Engine                  # noqa: E402
from ldweaver_amd.mi import make_blocks                 # noqa: E402
from ldweaver_amd.snpdat import SnpDat                  # noqa: E402
from ldweaver_amd.synth import synth_alignment          # noqa: E402


def main():
    out = {"reps": REPS, "block": BLK, "sr_dist": SR_DIST, "top": TOP, "lib": os.environ.get("LDW_AMD_LIB", ""), "copy_bytes_per_s": copy_rate(), "sizes": []}
    rate = out["copy_bytes_per_s"]
    with Engine(0) as eng:
        for N, Ls in SIZES:
            syn = synth_alignment(Ls, N, seed=N, device="cuda")
            eng.set_alignment(syn["states"])
            snp = SnpDat.from_states(None, syn["POS"], float(syn["g"]), counts=eng.state_counts())
            hdw = eng.hamming_weights(int(0.1 * Ls))
            eng.set_weights(hdw)
            eng.set_snp_meta(snp.r, snp.uqe, snp.POS, syn["paint"], snp.g)
            blocks = make_blocks(Ls, BLK)
            res, (_, ss_ms, _), ss_min, ss_max = timed(eng, lambda: eng.mi_snp_summary(blocks, SR_DIST))
            dres, (_, dec_ms, _), dec_min, dec_max = timed(eng, lambda: eng.mi_profile(blocks, default_cuts(snp.g), mi_shift=3))
            bg = B.SnpBackground(res["n"], res["sumq"], res["max"], res["nge"], res["npairs"], np.asarray(snp.POS), float(snp.g), SR_DIST, (np.inf, np.inf))
            w = B.apc_weights(bg, "lr")
            scan, (mi_ms, scan_ms, scan_wall), scan_min, scan_max = timed(eng, lambda: eng.mi_score_scan(blocks, SR_DIST, 2, w))
            thr, cap = B.pick_threshold(scan["hist"], TOP)
            lk, (_, links_ms, links_wall), links_min, links_max = timed(eng, lambda: eng.mi_score_links(blocks, SR_DIST, 2, w, thr, cap, best_in=scan["best"]))
            # (a timing-only ablation build, loaded through LDW_AMD_LIB, counts wrongly on purpose)
            assert out["lib"] or (lk["count"] == cap and scan["npairs"] == int(res["npairs"][1]) and int(scan["hist"].sum()) == scan["npairs"])
            walls = []
            for _ in range(1 + REPS):
                t0 = time.perf_counter()
                B.apc_links(snp, hdw, background=bg, top=TOP, sr_dist=SR_DIST, max_blk_sz=BLK, engine=eng, alignment_resident=True)
                walls.append((time.perf_counter() - t0) * 1e3)
            n, n_all = scan["npairs"], int(dres["n_pairs"])
            row = dict(sequences=N, snps=Ls, blocks=int(len(blocks)), pairs=n_all, pairs_long_range=n, blocks_gemm_epilogue_ms=round(mi_ms, 3),
                       score_scan_ms=round(scan_ms, 3), score_scan_min_ms=round(scan_min, 3), score_scan_max_ms=round(scan_max, 3),
                       score_links_ms=round(links_ms, 3), score_links_min_ms=round(links_min, 3), score_links_max_ms=round(links_max, 3),
                       snp_summary_ms=round(ss_ms, 3), snp_summary_min_ms=round(ss_min, 3), snp_summary_max_ms=round(ss_max, 3),
                       decay_hist_ms=round(dec_ms, 3), decay_hist_min_ms=round(dec_min, 3), decay_hist_max_ms=round(dec_max, 3),
                       score_links_over_snp_summary=round(links_ms / ss_ms, 3), score_scan_over_decay_plus_summary=round(scan_ms / (dec_ms + ss_ms), 3),
                       score_scan_read_bytes_per_s=8.0 * n_all / (scan_ms * 1e-3), score_scan_read_fraction_of_copy_rate=round(8.0 * n_all / (scan_ms * 1e-3) / rate, 4),
                       score_links_read_bytes_per_s=8.0 * n_all / (links_ms * 1e-3), score_links_read_fraction_of_copy_rate=round(8.0 * n_all / (links_ms * 1e-3) / rate, 4),
                       scan_call_wall_ms=round(scan_wall, 3), links_call_wall_ms=round(links_wall, 3), apc_links_call_wall_ms=round(float(np.median(walls[1:])), 3),
                       bucket_zero_share=round(int(scan["hist"][0]) / max(n, 1), 4), threshold=thr, cap=cap, patches=eng.score_select_report()["patches"],
                       overall_mean_lr=bg.overall_mean("lr"))
            out["sizes"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
