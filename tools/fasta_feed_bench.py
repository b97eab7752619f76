#!/usr/bin/env python3
"""Feed rate of the native FASTA reader (csrc/ldw_fasta.cpp) against the Python route, at config 3's alignment shape by default.

Writes a synthetic N x L alignment (60-character lines, a random reference with `--mut` of its sites changed per sequence) as plain text
and as gzip (level 1: deflate at level 6 takes minutes on 1.4 GB of such text) into a temporary directory, then measures, each in a
fresh child process (the page cache holds the files: they were just written):
  * native, filter: the whole native route of parse_fasta_alignment: Engine.fasta_scan, the host SNP filter (extract.snp_filter, whose
                    numpy temporaries are O(L_total): ~250 MB at 2.2 Mb), Engine.fasta_encode;
  * native, keep  : Engine.fasta_scan + Engine.fasta_encode of the columns the filter run retained, with the 4-bit packed copy on the
                    device (the file is read once) — the reader's own time and host memory;
  * native, reread: the same with keep_bytes = 0 (pass 2 reads the file again);
  * python        : parse_fasta_alignment(reader="python"): snpdat.read_fasta + the whole character matrix uploaded;
  * inflate       : a bare single-thread zlib inflate of the .gz (4 MiB reads), the floor of any single-stream gzip reader;
and per child the growth of its peak host RSS (VmHWM) over its RSS after a warm-up parse of a tiny file.  Prints one JSON document.

    python tools/fasta_feed_bench.py [--n 616] [--L 2200000] [--out profiles/fasta_feed.json] [--only plain:keep,gz:keep,...]
"""
import argparse
import gzip
import json
import os
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

_CHILD = r"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
from ldweaver_amd import extract
from ldweaver_amd.engine import Engine

def status():
    d = {}
    for line in open("/proc/self/status"):
        k, _, v = line.partition(":")
        if k in ("VmHWM", "VmRSS"):
            d[k] = int(v.split()[0]) * 1024
    return d

how, path, tiny, posfile = sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5]
eng = Engine(0)
extract.parse_fasta_alignment(tiny, engine=eng, keep_on_device=True)
extract.parse_fasta_alignment(tiny, engine=eng, keep_on_device=True, reader="python")
base = status()["VmRSS"]
out = {}
t0 = time.perf_counter()
if how == "python":
    sd = extract.parse_fasta_alignment(path, engine=eng, keep_on_device=True, reader="python")
    out["total_s"] = time.perf_counter() - t0
    out["n_pos"] = len(sd.POS)
else:
    names, ltot, counts = eng.fasta_scan(path, keep_bytes=0 if how == "reread" else -1)
    t1 = time.perf_counter()
    if how == "filter" or not os.path.exists(posfile):   # the host filter: O(L_total) numpy temporaries
        pos = extract.snp_filter(counts, len(names))
        np.save(posfile, pos)
    else:                                                 # the reader alone: the retained columns of an earlier run
        pos = np.load(posfile)
    t2 = time.perf_counter()
    eng.fasta_encode(pos)
    t3 = time.perf_counter()
    out.update(scan_s=t1 - t0, encode_s=t3 - t2, total_s=t3 - t0, scan_encode_s=(t1 - t0) + (t3 - t2), n_pos=len(pos))
    if how == "filter":
        out["filter_s"] = t2 - t1
out["rss_growth_MB"] = (status()["VmHWM"] - base) / 2**20
eng.close()
print(json.dumps(out))
"""


def write_alignment(d, n, ltot, mut, width, seed=2024):
    """-> (plain path, gz path, bytes of text).  One row at a time: the generator's own memory stays O(L)."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref = acgt[rng.integers(0, 4, size=ltot)]
    full = ltot // width * width
    plain, gzp = os.path.join(d, "aln.fa"), os.path.join(d, "aln.fa.gz")
    nbytes = 0
    with open(plain, "wb") as fp, gzip.open(gzp, "wb", compresslevel=1) as fz:
        for s in range(n):
            row = ref.copy()
            m = np.nonzero(rng.random(ltot) < mut)[0]
            row[m] = acgt[(np.searchsorted(acgt, row[m]) + rng.integers(1, 4, size=len(m))) % 4]
            body = np.hstack([row[:full].reshape(-1, width), np.full((full // width, 1), ord("\n"), dtype=np.uint8)]).tobytes()
            tail = row[full:].tobytes() + b"\n" if full < ltot else b""
            rec = b">genome_%05d\n" % s + body + tail
            fp.write(rec)
            fz.write(rec)
            nbytes += len(rec)
    return plain, gzp, nbytes


def bare_inflate(path, chunk=4 << 20):
    t0 = time.perf_counter()
    d = zlib.decompressobj(wbits=31)
    n = 0
    with open(path, "rb") as fh:
        while True:
            b = fh.read(chunk)
            if not b:
                break
            n += len(d.decompress(b))
    n += len(d.flush())
    return time.perf_counter() - t0, n


def child(how, path, tiny, posfile, timeout):
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, how, path, tiny, posfile], capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"child {how} {path} failed ({r.returncode}):\n{r.stderr[-3000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=616)
    ap.add_argument("--L", type=int, default=2_200_000)
    ap.add_argument("--mut", type=float, default=0.02)
    ap.add_argument("--width", type=int, default=60)
    ap.add_argument("--only", default="", help="comma-separated subset of plain:filter, plain:keep, plain:reread, plain:python, gz:keep, gz:reread, gz:python, "
                    "gz:inflate (without plain:filter the first native run filters for itself)")
    ap.add_argument("--timeout", type=float, default=900)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    runs = [("plain", "filter"), ("plain", "keep"), ("plain", "reread"), ("gz", "keep"), ("gz", "reread"), ("gz", "inflate"), ("plain", "python"),
            ("gz", "python")]
    if a.only:
        want = set(a.only.split(","))
        runs = [r for r in runs if f"{r[0]}:{r[1]}" in want]
    res = dict(n=a.n, L=a.L, mut=a.mut, width=a.width, runs={})
    with tempfile.TemporaryDirectory(prefix="fasta_feed_") as d:
        t0 = time.perf_counter()
        plain, gzp, nbytes = write_alignment(d, a.n, a.L, a.mut, a.width)
        res.update(text_bytes=nbytes, gz_bytes=os.path.getsize(gzp), write_s=time.perf_counter() - t0)
        tiny = os.path.join(d, "tiny.fa")
        with open(tiny, "w") as fh:
            fh.write(">a\nACGTACGTAA\n>b\nACGTACGTCC\n>c\nACGAACGTCA\n")
        for fmt, how in runs:
            path = plain if fmt == "plain" else gzp
            if how == "inflate":
                s, n = bare_inflate(gzp)
                assert n == nbytes
                r = dict(total_s=s)
            else:
                r = child(how, path, tiny, os.path.join(d, "pos.npy"), a.timeout)
            r["GBps_text"] = nbytes / r.get("scan_encode_s", r["total_s"]) / 1e9
            res["runs"][f"{fmt}:{how}"] = r
            print(f"{fmt:5s} {how:7s} " + " ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in r.items()), file=sys.stderr, flush=True)
    runs_ = res["runs"]
    if "gz:keep" in runs_ and "gz:inflate" in runs_:
        res["gz_keep_over_inflate"] = runs_["gz:keep"]["scan_encode_s"] / runs_["gz:inflate"]["total_s"]
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
