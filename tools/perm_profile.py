"""The permutation test for links timed on synthetic alignments, with the clusters the device finds at int(0.1 L).  Needs an MI355X.

    python tools/perm_profile.py [OUT.json] [N_SEQS:L_SNPS ...]      (defaults: profiles/perm.json, 5000:100000 616:85000)

Per size: the alignment of ldweaver_amd/synth.py made on the device and made resident, the clusters of ``Engine.seq_clusters(int(0.1 L))``, the Hamming
weights at the same threshold made resident, then ``Engine.links_permuted`` with N_PERM replicates for 250 and for 10^4 random pairs: one warm-up call,
REPS calls timed by the library's own HIP events (``Engine.last_timing()``: the pair kernel, keys and sorts, the copies out) and by the host's clock
around the call.  Recorded per run: the pair kernel's element rate, K B P positions per second; the bytes it reads from global memory per position —
the 4 of order_r[p], and the 8 of V[p] where the weights are not in LDS — as a share of the rate of a plain device copy (``torch`` ``copy_`` of 1 GiB,
read + written bytes per second) measured in the same run; and the sort's rate in keys per second.  The numpy restatement (tests/perm_ref.py
``links_permuted``) runs on the first REF_PAIRS pairs, on the host's clock, and is compared with the device within 1e-10; its time scaled to all pairs is
an extrapolation and is marked as one.  No time is required of the run; the file is where the measured numbers go."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "perm.json")
SIZES = [tuple(int(v) for v in x.split(":")) for x in sys.argv[2:]] or [(5000, 100000), (616, 85000)]
REPS = 5
REF_PAIRS = 2
N_PERM = 1000
PAIR_COUNTS = (250, 10000)
LDS_WITH_V = 80 * 1024            # csrc/ldw_perm.hip: the weights go to LDS while 64 + 8 P + Npad + P (rounded up to 16) stays within this
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import perm_ref                                        # noqa: E402
from ldweaver_amd.engine import Engine                 # noqa: E402
from ldweaver_amd.synth import synth_alignment         # noqa: E402
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
    """One warm-up, then REPS calls: medians (and the spread of the first) of the library's three event slots and of the host's clock, in ms."""
    call()
    rows = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        wall = (time.perf_counter() - t0) * 1e3
        t = eng.last_timing()
        rows.append((float(t["gemm_ms"]), float(t["epilogue_ms"]), float(t["select_ms"]), wall))
    rows = np.asarray(rows)
    m, lo, hi = np.median(rows, axis=0), rows.min(axis=0), rows.max(axis=0)
    return dict(pairs_ms=round(float(m[0]), 3), pairs_min_ms=round(float(lo[0]), 3), pairs_max_ms=round(float(hi[0]), 3), sorts_ms=round(float(m[1]), 3),
                copies_ms=round(float(m[2]), 3), call_wall_ms=round(float(m[3]), 3))


def main():
    out = {"reps": REPS, "n_perm": N_PERM, "copy_bytes_per_s": copy_rate(), "sizes": []}
    rate = out["copy_bytes_per_s"]
    rng = np.random.default_rng(1)
    with Engine(0) as eng:
        for N, Ls in SIZES:
            states = synth_alignment(Ls, N, seed=N, device="cuda")["states"]
            eng.set_alignment(states)
            thresh = int(0.1 * Ls)
            Npad = (N + 127) // 128 * 128
            labels, C = eng.seq_clusters(thresh)
            sizes = np.bincount(labels, minlength=C)
            hdw = eng.hamming_weights(thresh)
            eng.set_weights(hdw)
            P = N                                                  # every sequence has a cluster
            v_in_lds = 64 + 8 * P + Npad + (P + 15) // 16 * 16 <= LDS_WITH_V
            read_bytes = 4.0 + (0.0 if v_in_lds else 8.0)
            row = dict(sequences=N, snps=Ls, thresh=thresh, clusters=int(C), largest=sorted(sizes.tolist(), reverse=True)[:5], singletons=int((sizes == 1).sum()),
                       weights_in_lds=bool(v_in_lds), global_bytes_read_per_position=read_bytes, lds_bytes_per_workgroup=64 + (8 * P if v_in_lds else 0) + Npad + (P + 15) // 16 * 16)
            for K in PAIR_COUNTS:
                a, b = rng.integers(0, Ls, size=K).astype(np.int32), rng.integers(0, Ls, size=K).astype(np.int32)
                st = timed(eng, lambda: eng.links_permuted(a, b, labels, N_PERM, seed=1, C=C))
                elements = float(K) * N_PERM * P
                st.update(pairs=K, positions=elements, positions_per_s=round(elements / (st["pairs_ms"] * 1e-3), 0),
                          pairs_fraction_of_copy_rate=round(elements * read_bytes / (st["pairs_ms"] * 1e-3) / rate, 5),
                          ns_per_pair_replicate=round(st["pairs_ms"] * 1e6 / (float(K) * N_PERM), 2), sort_keys_per_s=round(float(N_PERM) * P / (st["sorts_ms"] * 1e-3), 0))
                if K == PAIR_COUNTS[0]:
                    # the numpy restatement on the first REF_PAIRS pairs: only the rows it reads come to the host
                    res = eng.links_permuted(a[:REF_PAIRS], b[:REF_PAIRS], labels, N_PERM, seed=1, C=C, want_null=True)
                    snps = np.unique(np.concatenate([a[:REF_PAIRS], b[:REF_PAIRS]]))
                    sub = states[torch.as_tensor(snps, device="cuda", dtype=torch.long)].cpu().numpy()
                    ra, rb = np.searchsorted(snps, a[:REF_PAIRS]), np.searchsorted(snps, b[:REF_PAIRS])
                    t0 = time.perf_counter()
                    ref = perm_ref.links_permuted(sub, hdw, ra, rb, labels, C, N_PERM, 1)
                    ref_s = time.perf_counter() - t0
                    err = max(float(np.abs(ref["null"] - res["null"]).max()), float(np.abs(ref["mi_obs"] - res["mi_obs"]).max()))
                    assert err < 1e-10, err
                    row["numpy_reference"] = dict(pairs=REF_PAIRS, replicates=N_PERM, seconds=round(ref_s, 2), max_abs_difference=err,
                                                  seconds_scaled_to_1e4_pairs_extrapolated=round(ref_s * 1e4 / REF_PAIRS, 0))
                row[f"permuted_{K}"] = st
            out["sizes"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
