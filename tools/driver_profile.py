"""One end-to-end run of the pipeline driver on a synthetic job of its own making, and the kernel times of one xy figure.
Needs an MI355X.

    python tools/driver_profile.py [OUT.json] [SCRATCH_DIR] [L_SNPS] [N_SEQS]      (defaults: profiles/driver_run.json, a temporary directory, 20000, 1000)

The job: a synthetic alignment (ldweaver_amd/synth.py) written as a SNP-only FASTA with its positions through snpdat_to_fa, a random reference of
the genome's length and a generated GFF3 of CDSs tiled over it.  No time is required of the run; the file is where the first measured number goes."""
import json
import os
import sys
import tempfile
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "driver_run.json")
TMP = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp(prefix="ldw_driver_")
L_SNPS = int(sys.argv[3]) if len(sys.argv) > 3 else 20000
N_SEQS = int(sys.argv[4]) if len(sys.argv) > 4 else 1000
sys.path.insert(0, ROOT)
from ldweaver_amd import _lib as L                     # noqa: E402
from ldweaver_amd import LDWeaver, plots as P          # noqa: E402
from ldweaver_amd.engine import Engine                 # noqa: E402
from ldweaver_amd.output import snpdat_to_fa           # noqa: E402
from ldweaver_amd.snpdat import SnpDat                 # noqa: E402
from ldweaver_amd.synth import synth_alignment         # noqa: E402

os.makedirs(TMP, exist_ok=True)
out = {"job": {"snps": L_SNPS, "sequences": N_SEQS}}

# ---- the xy kernels, for completeness: the fit figure's panel at its largest input
lay = P.layout(L.PLOT_FIT)
W, H = lay["panel_w"], lay["panel_h"]
rng = np.random.default_rng(3)
with Engine(0) as eng:
    rows = []
    for n, nv in ((100_000, 100_000), (5_000, 0)):
        ln = np.arange(1.0, n + 1)
        mx = 0.3 * np.exp(-ln / (n / 5)) + 0.03 + rng.normal(0, 0.004, n)
        line = (ln[:nv], (0.3 * np.exp(-ln / (n / 5)) + 0.03)[:nv]) if nv else None
        cls = None if nv else rng.integers(0, 3, n).astype(np.uint8)
        o = P.xy_opts(L.PLOT_FIT if nv else L.PLOT_CDS, class_rgb=[0] if nv else [0xF8766D, 0x00BA38, 0x619CFF])
        for _ in range(3):
            _, st, ms = P.debug_xy_panel(eng, ln, mx, cls, line, opts=o, W=W, H=H, timing=True)
        rows.append(dict(points=n, vertices=nv, **{k: round(float(v), 4) for k, v in ms.items()}))
out["xy_panel_ms"] = {"panel": [W, H], "runs": rows}

# ---- the job
t0 = time.time()
g = 2_221_315
syn = synth_alignment(L_SNPS, N_SEQS, g=g)
names = [f"iso_{k}" for k in range(N_SEQS)]
sd = SnpDat.from_states(syn["states"], syn["POS"], g=float(g), seq_names=names)
aln, pos_path = os.path.join(TMP, "job.fa"), os.path.join(TMP, "job.pos")
for p in (aln, pos_path):
    if os.path.exists(p):
        os.remove(p)
snpdat_to_fa(sd, aln, pos_path)
ref = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), g)
ref_path, gff_path = os.path.join(TMP, "job_ref.fa"), os.path.join(TMP, "job.gff3")
with open(ref_path, "wb") as fh:
    fh.write(b">synth\n" + ref.tobytes() + b"\n")
with open(gff_path, "w") as fh:
    fh.write("##gff-version 3\n")
    at, i = 101, 0
    while at + 1300 < g:
        ln_ = 3 * int(rng.integers(150, 400))
        fh.write(f"synth\tsynth\tCDS\t{at}\t{at + ln_ - 1}\t.\t{'+' if i % 2 else '-'}\t0\tID=cds{i};Name=gene{i};locus_tag=SY_{i:05d}\n")
        at += ln_ + int(rng.integers(30, 400))
        i += 1
out["job"].update(genome=g, cds=i, make_s=round(time.time() - t0, 2))
pos = np.loadtxt(pos_path, dtype=np.int64)
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    res = LDWeaver(os.path.join(TMP, "dset"), aln, aln_has_all_bases=False, pos=pos, gff3_path=gff_path, ref_fasta_path=ref_path, verbose=False)
out["timings_s"] = {k: round(float(v), 3) for k, v in res["timings"].items()}
out["files"] = sorted(res["files"])
with open(OUT, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps(out["timings_s"]))
