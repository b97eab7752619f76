"""The lineage check timed on synthetic alignments, with the clusters the device finds at int(0.1 L).  Needs an MI355X.

    python tools/lineage_profile.py [OUT.json] [N_SEQS:L_SNPS ...]      (defaults: profiles/lineage.json, 5000:100000 616:85000)

Per size: the alignment of ldweaver_amd/synth.py made on the device and made resident, then
  * ``Engine.seq_clusters(int(0.1 L))``: one warm-up call, REPS calls timed by the library's own HIP events (``Engine.last_timing()``: the rounds, what
    ran in front of them, the rounds taken) and by the host's clock around the call;
  * the Hamming weights at the same threshold made resident, and ``Engine.links_stratified`` for 250 and for 10^6 random pairs on those clusters, the same
    way (the bit rows, the pairs, the copies out);
  * the numpy restatement (tests/lineage_ref.py ``links_stratified``) on the first REF_PAIRS pairs, on the host's clock, compared with the device within
    1e-10, and that time scaled to all pairs (its loop is over the pairs: the scaling is an extrapolation and is marked as one).
The bytes a kernel moves are counted from the statement — k_clu_adj reads the lower triangle of G twice and writes N x Npad bits; a round of k_clu_hook
reads the adjacency bits once and one f per set bit; k_lin_bits reads, per distinct SNP, a byte and a permutation entry per labelled sequence and writes
five bit rows; k_lin_pairs reads, per pair, the rows of the states its two SNPs show and the pieces, and writes C x 9 + 8 bytes — and set against the
rate of a plain device copy (``torch`` ``copy_`` of 1 GiB, read + written bytes per second) measured in the same run.  No time is required of the run;
the file is where the measured numbers go."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lineage.json")
SIZES = [tuple(int(v) for v in x.split(":")) for x in sys.argv[2:]] or [(5000, 100000), (616, 85000)]
REPS = 5
REF_PAIRS = 50
PAIR_COUNTS = (250, 1000000)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lineage_ref                                     # noqa: E402
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


def timed(eng, call, names):
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
    out = {names[k]: round(float(m[k]), 3) for k in range(3)}
    out.update({names[0].replace("_ms", "_min_ms"): round(float(lo[0]), 3), names[0].replace("_ms", "_max_ms"): round(float(hi[0]), 3), "call_wall_ms": round(float(m[3]), 3)})
    return out


def main():
    out = {"reps": REPS, "copy_bytes_per_s": copy_rate(), "sizes": []}
    rate = out["copy_bytes_per_s"]
    rng = np.random.default_rng(1)
    with Engine(0) as eng:
        for N, Ls in SIZES:
            states = synth_alignment(Ls, N, seed=N, device="cuda")["states"]
            eng.set_alignment(states)
            thresh = int(0.1 * Ls)
            Npad = (N + 127) // 128 * 128
            row = dict(sequences=N, snps=Ls, thresh=thresh)
            cl = timed(eng, lambda: eng.seq_clusters(thresh), ("rounds_ms", "front_ms", "rounds"))
            labels, C = eng.seq_clusters(thresh)
            sizes = np.bincount(labels, minlength=C)
            edges = 1.0 / eng.hamming_weights(thresh) - 1.0          # the neighbours of every sequence, itself among them
            adj_bytes, set_bits = float(N) * Npad / 8.0, float(np.rint(edges).sum())
            round_bytes = adj_bytes + 4.0 * set_bits + 8.0 * N
            cl.update(clusters=int(C), largest=sorted(sizes.tolist(), reverse=True)[:5], singletons=int((sizes == 1).sum()), adjacency_bytes=adj_bytes, set_bits=set_bits,
                      bytes_per_round=round_bytes, rounds_fraction_of_copy_rate=round(round_bytes * cl["rounds"] / (cl["rounds_ms"] * 1e-3) / rate, 5),
                      front_bytes_after_the_gemm=float(N) * N * 8.0 + adj_bytes)
            row["clusters"] = cl
            hdw = eng.hamming_weights(thresh)
            eng.set_weights(hdw)
            W = (N + 63) // 64
            for K in PAIR_COUNTS:
                a, b = rng.integers(0, Ls, size=K).astype(np.int32), rng.integers(0, Ls, size=K).astype(np.int32)
                distinct = int(len(np.unique(np.concatenate([a, b]))))
                st = timed(eng, lambda: eng.links_stratified(a, b, labels, C), ("pairs_ms", "bits_ms", "copies_ms"))
                res = eng.links_stratified(a, b, labels, C)
                bits_bytes = float(distinct) * (N + 4.0 * N + 5.0 * W * 8.0)
                pair_bytes = float(K) * (2.0 * 2.0 * W * 8.0 + C * 9.0 + 8.0)      # (two states per SNP, the common case of the synthetic alignment)
                st.update(pairs=K, distinct_snps=distinct, bits_bytes=bits_bytes, bits_fraction_of_copy_rate=round(bits_bytes / (st["bits_ms"] * 1e-3) / rate, 5),
                          pair_bytes_two_states_per_snp=pair_bytes, pairs_fraction_of_copy_rate=round(pair_bytes / (st["pairs_ms"] * 1e-3) / rate, 5),
                          ns_per_pair=round(st["pairs_ms"] * 1e6 / K, 1), output_bytes=float(K) * (C * 9.0 + 8.0))
                if K == PAIR_COUNTS[0]:
                    # the numpy restatement on the first REF_PAIRS pairs: only the rows it reads come to the host
                    k = min(REF_PAIRS, K)
                    snps = np.unique(np.concatenate([a[:k], b[:k]]))
                    sub = states[torch.as_tensor(snps, device="cuda", dtype=torch.long)].cpu().numpy()
                    ra, rb = np.searchsorted(snps, a[:k]), np.searchsorted(snps, b[:k])
                    t0 = time.perf_counter()
                    ref = lineage_ref.links_stratified(sub, hdw, ra, rb, labels, C)
                    ref_s = time.perf_counter() - t0
                    err = max(float(np.abs(ref["mi"] - res["mi"][:k]).max()), float(np.abs(ref["mi_all"] - res["mi_all"][:k]).max()))
                    assert err < 1e-10 and np.array_equal(ref["poly"], res["poly"][:k]), err
                    row["numpy_reference"] = dict(pairs=k, seconds=round(ref_s, 2), max_abs_difference=err,
                                                  seconds_scaled_to_1e6_pairs_extrapolated=round(ref_s * 1e6 / k, 0))
                row[f"stratified_{K}"] = st
                del res
            out["sizes"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
