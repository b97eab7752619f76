"""Times of the native link-table reader on a 1e7-row sr_links.tsv written by the library's writer, plain and gzip, with a warm page
cache: file to device columns and its stages, against the two yardsticks measured in the same run — pandas' read_csv as plots.read_ShortRangeLinks calls
it, and a bare gzread loop over the file that parses nothing — and make_gwes_plots file to PNG under both readers.  Needs an MI355X.

    python tools/links_read_profile.py [OUT.json] [SCRATCH_DIR] [ROWS]      (defaults: profiles/links_read.json, a temporary directory, 1e7)

2 warm-up calls, then the median of 5.  Every host timer encloses a synchronise (the library's calls return after theirs)."""
import ctypes
import ctypes.util
import gzip
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "links_read.json")
TMP = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="ldw_links_")
N = int(float(sys.argv[3])) if len(sys.argv) > 3 else 10_000_000
sys.path.insert(0, ROOT)
from ldweaver_amd import _lib as L          # noqa: E402
from ldweaver_amd import plots as P         # noqa: E402
from ldweaver_amd.engine import Engine, write_table_tsv   # noqa: E402


def timed(fn, warm=2, reps=5):
    v = []
    for rep in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        if rep >= warm:
            v.append(time.perf_counter() - t0)
    return float(np.median(v)), [round(x, 4) for x in v]


def bare_read(path):
    """zlib's gzread over the whole file in 64-MiB calls: what the reader's host side cannot go below."""
    z = ctypes.CDLL(ctypes.util.find_library("z") or "libz.so.1")
    z.gzopen.restype = ctypes.c_void_p
    z.gzopen.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    z.gzread.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint]
    z.gzclose.argtypes = [ctypes.c_void_p]
    z.gzbuffer.argtypes = [ctypes.c_void_p, ctypes.c_uint]
    buf = ctypes.create_string_buffer(64 << 20)

    def run():
        f = z.gzopen(os.fsencode(path), b"rb")
        z.gzbuffer(f, 1 << 20)
        while z.gzread(f, buf, 64 << 20) > 0:
            pass
        z.gzclose(f)
    return run


os.makedirs(TMP, exist_ok=True)
rng = np.random.default_rng(7)
x = np.floor(rng.random(N) * 50000.0) + 1.0
clust = (np.arange(N) % 3 + 1).astype(np.int32)
cols = [clust, x.astype(np.int32), (x + 17).astype(np.int32), clust, clust, x, rng.random(N) ** 4, 3.0 - 4.0 * np.log1p(-rng.random(N)), (rng.random(N) < 0.7).astype(np.int32)]
plain, gz = os.path.join(TMP, "sr_links.tsv"), os.path.join(TMP, "sr_links.tsv.gz")
write_table_tsv(plain, cols, append=False)
with open(plain, "rb") as f, gzip.open(gz, "wb", compresslevel=1) as g:
    shutil.copyfileobj(f, g, 16 << 20)
del cols, x
out = {"rows": N, "tsv_bytes": os.path.getsize(plain), "gz_bytes": os.path.getsize(gz), "warm_up_calls": 2, "timed_calls": 5}

out["pandas_read_csv_s"], out["pandas_read_csv_all_s"] = timed(lambda: P.read_ShortRangeLinks(plain))
out["bare_gzread_plain_s"], _ = timed(bare_read(plain))
out["bare_gzread_gz_s"], _ = timed(bare_read(gz))
print(json.dumps(out), flush=True)

with Engine(0) as eng:
    def native(path, variant):
        L.check(L.lib().ldw_tsv_set_variant(eng._ctx, variant))
        stats = []

        def run():
            rows, slow, _ = eng.tsv_read(path, "\t", 9)
            assert rows == N and slow == 0
            stats.append(eng.tsv_stats())
        med, allv = timed(run)
        st = {k: float(np.median([s[k] for s in stats[2:]])) for k in ("read_ms", "copy_ms", "line_ms", "parse_ms", "patch_ms")}
        st.update(file_to_columns_s=med, all_s=allv, chunks=stats[-1]["chunks"], grows_total=stats[-1]["grows"],
                  parse_GBps=stats[-1]["bytes"] / (st["parse_ms"] * 1e-3) / 1e9)
        return st
    # the two forms of the parse kernel, alternating
    out["native_plain_global_loads"] = native(plain, 0)
    out["native_plain_lds_tile"] = native(plain, 1)
    out["native_plain_global_loads_again"] = native(plain, 0)
    best = 0 if out["native_plain_global_loads_again"]["parse_ms"] <= out["native_plain_lds_tile"]["parse_ms"] else 1
    out["native_gz"] = native(gz, best)
    L.check(L.lib().ldw_tsv_set_variant(eng._ctx, best))
    # yardstick of the parse kernel: a torch device copy of one chunk
    src = torch.empty(64 << 20, dtype=torch.uint8, device="cuda").random_(0, 255)
    dst = torch.empty_like(src)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    cp = []
    for rep in range(7):
        ev[0].record()
        dst.copy_(src)
        ev[1].record()
        torch.cuda.synchronize()
        if rep >= 2:
            cp.append(ev[0].elapsed_time(ev[1]))
    out["device_copy_64MiB_ms"] = float(np.median(cp))
    out["device_copy_read_GBps"] = (64 << 20) / (out["device_copy_64MiB_ms"] * 1e-3) / 1e9
    del src, dst
    print(json.dumps(out), flush=True)
    # the LD map's accumulation: values below 64 go through the order-independent fixed-point accumulators (two integer atomics per link), values from
    # 64 up through the fp64 atomic add every value took before — the same table shifted by 64 times the old path
    nl, Lp = 10_000_000, 100_000
    eng.set_positions((np.arange(Lp, dtype=np.int32) + 1) * 40, 0.0)
    la, lb, lmi = rng.integers(0, Lp, nl).astype(np.int32), rng.integers(0, Lp, nl).astype(np.int32), rng.random(nl)
    for name, shift in (("ldmap_fixed_point_s", 0.0), ("ldmap_fp64_atomics_s", 64.0)):
        eng.links_import(1, la, lb, lmi + shift)
        out[name], _ = timed(lambda: eng.ldmap(100))
    out["ldmap_links"], out["ldmap_cells"] = nl, (Lp // 100) ** 2
    eng.links_import(1, la[:1], lb[:1], lmi[:1])
    print(json.dumps(out), flush=True)
    for reader in ("pandas", "native"):
        folder = os.path.join(TMP, "P_" + reader)
        out[f"make_gwes_plots_{reader}_s"], out[f"make_gwes_plots_{reader}_all_s"] = timed(
            lambda: P.make_gwes_plots(sr_links=plain, plt_folder=folder, engine=eng, reader=reader), warm=1, reps=3)
    a, b = (open(os.path.join(TMP, "P_" + r, "sr_gwes_combi.png"), "rb").read() for r in ("pandas", "native"))
    out["figures_identical"] = a == b
out["native_faster_than_pandas"] = out["native_plain_global_loads_again" if best == 0 else "native_plain_lds_tile"]["file_to_columns_s"] < out["pandas_read_csv_s"]
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
for p in (plain, gz):
    os.remove(p)
assert out["native_faster_than_pandas"], "the plain-file native read must be faster than the pandas read of the same run"
