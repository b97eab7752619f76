"""Mirror of ``estimate_variation_in_CDS`` (R/estimateCDSDiversity.R:27-210) and ``parse_gff_file`` (R/parseGFF.R:19-32).

The annotation (CDS intervals + reference sequence) and the resident alignment give ``cds_var``, the argument ``perform_MI_computation``
takes: per SNP the non-reference state counts, per CDS the variation per base, a k-means clustering of the CDSs and the paint of every SNP.
The annotation comes from GFF3 plus a reference FASTA (``parse_gff_file``, the FASTA's case kept) or from a GenBank file
(``parse_genbank_file`` in gbk.py, native parser csrc/ldw_gbk.cpp, sequence upper case).  The per-SNP and per-CDS work runs on the device
(``Engine.cds_variation`` / ``Engine.cds_paint``, csrc/ldw_cds.hip); the clustering of the kept CDSs is the exact 1-D optimum on the host
(``kmeans_1d``).  The cluster plot is not drawn.
"""
from __future__ import annotations

import gzip
import os
import warnings
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from .engine import Engine, kmeans_1d
from .snpdat import CdsVar, SnpDat

_ALPHA = ("A", "C", "G", "T", "*")
_ALT_OF_MASK = [",".join(_ALPHA[x] for x in range(5) if (m >> x) & 1) for m in range(32)]


@dataclass
class Annotation:
    """What ``parse_gff_file`` returns: ``gff`` the feature table (columns seqid, source, type, start, end, score, strand, phase,
    attributes; start / end int64), ``ref`` the reference sequence as uint8 characters (case preserved), its name and length ``g``."""
    gff: object              # pandas.DataFrame
    ref: np.ndarray
    ref_name: str
    g: int
    gff_path: str | None = None
    ref_path: str | None = None

    @classmethod
    def from_arrays(cls, starts, ends, ref, ref_name: str = "ref"):
        """An annotation whose features are the CDSs [starts[j], ends[j]] (1-based, inclusive) on the reference ``ref`` (str, bytes or
        uint8 characters)."""
        import pandas as pd
        st = np.asarray(starts, dtype=np.int64).ravel()
        en = np.asarray(ends, dtype=np.int64).ravel()
        if st.shape != en.shape:
            raise ValueError("starts and ends differ in length")
        r = _as_chars(ref)
        n = len(st)
        gff = pd.DataFrame({"seqid": [ref_name] * n, "source": ["."] * n, "type": ["CDS"] * n, "start": st, "end": en,
                            "score": ["."] * n, "strand": ["+"] * n, "phase": ["0"] * n, "attributes": [""] * n})
        return cls(gff=gff, ref=r, ref_name=ref_name, g=len(r))


def _as_chars(ref) -> np.ndarray:
    if isinstance(ref, str):
        ref = ref.encode("ascii")
    if isinstance(ref, (bytes, bytearray)):
        return np.frombuffer(bytes(ref), dtype=np.uint8).copy()
    a = np.asarray(ref)
    if a.dtype.kind in ("U", "S"):
        return np.frombuffer("".join(a.astype(str).tolist()).encode("ascii"), dtype=np.uint8).copy()
    return np.ascontiguousarray(a, dtype=np.uint8).ravel()


def _open(path):
    return gzip.open(path, "rb") if str(path).endswith(".gz") else open(path, "rb")


def read_gff3(gff3_path):
    """GFF3 feature lines up to a ``##FASTA`` trailer (comment and blank lines skipped, CRLF accepted) as a DataFrame of the nine columns."""
    import pandas as pd
    if not os.path.exists(gff3_path):
        raise FileNotFoundError(f"{gff3_path} not found!")
    cols = [[] for _ in range(9)]
    with _open(gff3_path) as fh:
        for lineno, raw in enumerate(fh, 1):
            line = raw.decode("utf-8", "replace").rstrip("\r\n")
            if line.startswith("##FASTA"):
                break
            if not line.strip() or line.startswith("#"):
                continue
            f = line.split("\t")
            if len(f) != 9:
                raise ValueError(f"{gff3_path}: line {lineno}: a GFF3 feature line has 9 tab-separated fields, found {len(f)}")
            try:
                f[3], f[4] = int(f[3]), int(f[4])
            except ValueError:
                raise ValueError(f"{gff3_path}: line {lineno}: start and end must be integers") from None
            for c, v in zip(cols, f):
                c.append(v)
    names = ("seqid", "source", "type", "start", "end", "score", "strand", "phase", "attributes")
    df = pd.DataFrame({n: c for n, c in zip(names, cols)})
    df["start"] = df["start"].astype(np.int64)
    df["end"] = df["end"].astype(np.int64)
    return df


def read_reference_fasta(ref_fasta_path):
    """(name, uint8 characters) of the FIRST record of a (gz) FASTA file (read_ReferenceFasta, R/io_functions.R:177-195)."""
    if not os.path.exists(ref_fasta_path):
        raise FileNotFoundError(f"{ref_fasta_path} not found!")
    name, parts = None, []
    with _open(ref_fasta_path) as fh:
        for raw in fh:
            line = raw.rstrip(b"\r\n")
            if line.startswith(b">"):
                if name is not None:
                    break
                name = line[1:].split()[0].decode() if len(line) > 1 and line[1:].split() else ""
            elif name is not None:
                parts.append(line.strip())
    seq = b"".join(parts)
    if name is None or len(seq) == 0:
        raise ValueError("empty sequence!")
    return name, np.frombuffer(seq, dtype=np.uint8).copy()


def parse_gff_file(gff3_path, ref_fasta_path, perform_length_check=True) -> Annotation:
    """Mirror of ``parse_gff_file`` (R/parseGFF.R:19-32): the GFF3 features and the reference's first FASTA record, with the reference's
    three length checks (R/parseGFF.R:23-28) over every feature."""
    name, ref = read_reference_fasta(ref_fasta_path)
    gff = read_gff3(gff3_path)
    g = len(ref)
    if perform_length_check and len(gff):
        se = np.concatenate([gff["start"].to_numpy(), gff["end"].to_numpy()])
        if se.min() < 0:
            raise ValueError("Invalid start position found!")
        if se.max() > g:
            raise ValueError("Invalid stop position found!")
        if np.any(gff["end"].to_numpy() < gff["start"].to_numpy()):
            raise ValueError("Invalid start-stop pair found!")
    return Annotation(gff=gff, ref=ref, ref_name=name, g=g, gff_path=str(gff3_path), ref_path=str(ref_fasta_path))


def estimate_variation_in_CDS(snp_dat: SnpDat, ncores=1, gbk=None, gff: Annotation | None = None, num_clusts_CDS=3, clust_plt_path=None,
                              mega_dset=False, *, engine: Engine | None = None, alignment_resident: bool = False,
                              quirk_mode: int = L.QUIRK_REFERENCE) -> CdsVar:
    """Mirror of ``estimate_variation_in_CDS`` with an annotation from ``parse_gff_file`` or ``Annotation.from_arrays`` (``gff``), or from
    ``parse_genbank_file`` (``gbk``: the dict it returns or its GenBankRecord; starts and ends of every CDS row, the upper-case sequence).

    ``engine`` with ``alignment_resident=True``: the engine already holds ``snp_dat``'s alignment (e.g. ``parse_fasta_alignment(...,
    keep_on_device=True)``).  The clustering is the exact optimum of the k-means objective (``kmeans_1d``) where the reference draws
    ``stats::kmeans(nstart = 10)`` from an unseeded RNG.  ``quirk_mode``: QUIRK_REFERENCE reproduces painter's loop, which leaves a last run
    of one SNP unrecorded (an unpainted such SNP keeps 0, and a UserWarning names it); QUIRK_INTENDED fills it from the left.
    ``clust_plt_path``: where ``CDS_clustering.png`` is drawn (``plots.cds_cluster_plot``); None draws nothing — the reference's default file
    ``clust_plt.png`` in the working directory is deliberately not reproduced.  ``ncores`` and ``mega_dset`` are accepted and ignored."""
    if (gbk is None) == (gff is None):
        raise ValueError("Provide either one of gbk or gff")
    if gbk is not None:
        from .gbk import GenBankRecord
        rec = gbk.get("gbk") if isinstance(gbk, dict) else gbk
        if not isinstance(rec, GenBankRecord):
            raise NotImplementedError("gbk must be what parse_genbank_file returns (or its GenBankRecord); other GenBank objects are not supported")
        starts = np.asarray(rec.cds["start"]).astype(np.int64)      # gbk@cds: every CDS row (R/estimateCDSDiversity.R:40-43)
        ends = np.asarray(rec.cds["end"]).astype(np.int64)
        ref = rec.sequence
    else:
        typ = np.asarray(gff.gff["type"]).astype(str)
        is_cds = np.char.lower(typ) == "cds"
        starts = np.asarray(gff.gff["start"])[is_cds].astype(np.int64)
        ends = np.asarray(gff.gff["end"])[is_cds].astype(np.int64)
        ref = gff.ref
    lim = np.iinfo(np.int32)
    if len(starts) and (min(starts.min(), ends.min()) < lim.min or max(starts.max(), ends.max()) > lim.max):
        raise ValueError("CDS bounds must fit in 32 bits")
    ref_seq = _as_chars(ref)
    own = engine is None
    eng = engine or Engine(0)
    try:
        if not alignment_resident:
            eng.set_alignment(snp_dat.states)
        var, _snp_var, alt_mask, refc = eng.cds_variation(snp_dat.POS, ref_seq, starts, ends)
        allele_table = eng.state_counts()
        keep = ~np.isnan(var)
        var_estimate, cds_start, cds_end = var[keep], starts[keep], ends[keep]
        labels, cutoff = kmeans_1d(var_estimate, int(num_clusts_CDS))
        paint, n0 = eng.cds_paint(cds_start, cds_end, labels, int(num_clusts_CDS), quirk_mode)
    finally:
        if own:
            eng.close()
    if n0 > 0:
        idx = np.flatnonzero(paint == 0)
        warnings.warn(f"SNP {int(idx[0])} (POS {int(np.asarray(snp_dat.POS)[idx[0]])}) keeps paint 0: it is the last SNP, alone in its run, and "
                      "painter does not record that run (R/estimateCDSDiversity.R:166-178); perform_MI_computation's short-range model "
                      "rejects paint 0.  quirk_mode=QUIRK_INTENDED paints it from the left.", UserWarning, stacklevel=2)
    cv = CdsVar(paint=paint, nclust=int(num_clusts_CDS), var_estimate=var_estimate, cds_start=cds_start, cds_end=cds_end,
                clusts={"km_clst_ord": labels, "cutoff": cutoff}, ref=refc.view("S1").astype("U1"),
                alt=[_ALT_OF_MASK[m] for m in alt_mask.tolist()], allele_table=allele_table)
    if clust_plt_path is not None:
        from .plots import cds_cluster_plot
        cds_cluster_plot(cv, clust_plt_path, engine=engine)
    return cv
