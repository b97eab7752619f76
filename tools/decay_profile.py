"""The LD-decay profile timed on synthetic alignments.  Needs an MI355X.

    python tools/decay_profile.py [OUT.json] [N_SEQS:L_SNPS ...]      (defaults: profiles/decay.json, 5000:100000 616:85000)

Per size: the alignment of ldweaver_amd/synth.py made on the device and made resident, its Hamming weights at int(0.1 L) and its SNP meta data set, then
``Engine.mi_profile`` over ``make_blocks(L, 10000)`` with ``default_cuts(g)`` and mi_shift 3: one warm-up call, REPS calls timed by the library's own HIP
events (``Engine.last_timing()``: the blocks' GEMM + epilogue, the histogram kernels) and by the host's clock around the call.  Recorded:
  * k_decay_hist over the call and per 10^8 pairs (a full 10 000 x 10 000 block), and the bytes it reads — 8 per pair — per second against the rate of a
    plain device copy (``torch`` ``copy_`` of 1 GiB, read + written bytes per second) measured in the same run;
  * the share of its patches that took route B (``Engine.decay_report()``), and the pairs found outside their patch's bound (0 for an integral g);
  * the whole call against the sum of its blocks' GEMM + epilogue time: what the profile costs on top of producing the values.
No time is required of the run; the file is where the measured numbers go."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "decay.json")
SIZES = [tuple(int(v) for v in x.split(":")) for x in sys.argv[2:]] or [(5000, 100000), (616, 85000)]
REPS = 5
BLK = 10000
MI_SHIFT = 3
sys.path.insert(0, ROOT)
from ldweaver_amd.decay import LDDecay, default_cuts    # noqa: E402
from ldweaver_amd.engine import Engine                  # noqa: E402
from ldweaver_amd.mi import make_blocks                 # noqa: E402
from ldweaver_amd.snpdat import SnpDat                  # noqa: E402
from ldweaver_amd.synth import synth_alignment          # noqa: E402
import torch                                            # noqa: E402


def copy_rate() -> float:
    """Bytes read + written per second by a device-to-device copy of 1 GiB (the best of 5 after a warm-up), as tools/lineage_profile.py measures it."""
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


def main():
    out = {"reps": REPS, "block": BLK, "mi_shift": MI_SHIFT, "copy_bytes_per_s": copy_rate(), "sizes": []}
    rate = out["copy_bytes_per_s"]
    with Engine(0) as eng:
        for N, Ls in SIZES:
            syn = synth_alignment(Ls, N, seed=N, device="cuda")
            eng.set_alignment(syn["states"])
            snp = SnpDat.from_states(None, syn["POS"], float(syn["g"]), counts=eng.state_counts())
            eng.set_weights(eng.hamming_weights(int(0.1 * Ls)))
            eng.set_snp_meta(snp.r, snp.uqe, snp.POS, syn["paint"], snp.g)
            blocks, cuts = make_blocks(Ls, BLK), default_cuts(snp.g)
            res = eng.mi_profile(blocks, cuts, mi_shift=MI_SHIFT)                       # the warm-up call
            rows = []
            for _ in range(REPS):
                t0 = time.perf_counter()
                res = eng.mi_profile(blocks, cuts, mi_shift=MI_SHIFT)
                wall = (time.perf_counter() - t0) * 1e3
                t = eng.last_timing()
                rows.append((float(t["gemm_ms"]), float(t["epilogue_ms"]), wall))
            rows = np.asarray(rows)
            mi_ms, hist_ms, wall_ms = (float(v) for v in np.median(rows, axis=0))
            rep, n = eng.decay_report(), res["n_pairs"]
            dec = LDDecay(res["hist"], res["max"], cuts, snp.g, MI_SHIFT, n)
            read_rate = 8.0 * n / (hist_ms * 1e-3)
            row = dict(sequences=N, snps=Ls, blocks=int(len(blocks)), cuts=int(len(cuts)), pairs=int(n),
                       blocks_gemm_epilogue_ms=round(mi_ms, 3), hist_ms=round(hist_ms, 3), hist_min_ms=round(float(rows[:, 1].min()), 3),
                       hist_max_ms=round(float(rows[:, 1].max()), 3), call_wall_ms=round(wall_ms, 3),
                       hist_ms_per_1e8_pairs=round(hist_ms * 1e8 / n, 4), hist_read_bytes_per_s=read_rate,
                       hist_read_fraction_of_copy_rate=round(read_rate / rate, 4), hist_share_of_gemm_epilogue=round(hist_ms / mi_ms, 4),
                       wall_over_gemm_epilogue=round(wall_ms / mi_ms, 3), patches=rep["patches"], route_b_patches=rep["route_b"],
                       route_b_share=round(rep["route_b"] / max(rep["patches"], 1), 5), pairs_outside_their_bound=rep["outside"],
                       pairs_per_s_whole_call=n / (wall_ms * 1e-3))
            try:
                row["suggested_sr_dist"] = dec.suggest_sr_dist()
                row["background_q95"] = dec.background(0.95)[0]
            except ValueError as e:
                row["suggested_sr_dist"] = str(e)
            out["sizes"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
