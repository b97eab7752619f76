"""The SNP alignment files: ``snpdat_to_fa`` (R/io_functions.R:363-417), ``generate_Links_SNPS_fasta`` (:432-460), ``read_TopHits`` (:13-16),
``read_AnnotatedLinks`` (:80-83) and ``write_output_for_gwes_explorer`` (R/createGWESExplorerOutput.R:23-76).

The FASTA records and the tsv body are rendered from the resident states on the device and streamed out in chunks (``Engine.write_alignment``,
csrc/ldw_out.hip): host memory stays O(chunk) whatever N and L are, so ``parse_fasta_alignment(..., keep_on_device=True)`` inputs are written
without a host copy of the states.  Every function takes ``engine`` / ``alignment_resident`` as ``estimate_variation_in_CDS`` does; without an
engine one is made, ``snp_dat.states`` uploaded and the engine closed.  Every argument check runs before an engine is made.  Positions always
print as integers and inputs R would fail on obscurely raise a ValueError that names the cause.
"""
from __future__ import annotations

import csv
import os
import warnings

import numpy as np

from . import rcompat
from .engine import Engine
from .snpdat import SnpDat

OUTLIER_COLS = ("Pos_1", "Pos_2", "Distance", "Direct", "MI", "MI_wogaps")


def read_TopHits(top_hits_path):
    """``read.table(top_hits_path, sep = "\\t", header = T, quote = "", comment.char = "")`` as a pandas DataFrame."""
    import pandas as pd
    return pd.read_csv(top_hits_path, sep="\t", header=0, quoting=csv.QUOTE_NONE)


def read_AnnotatedLinks(annotated_links_path):
    """``read.table(annotated_links_path, sep = "\\t", quote = "", comment.char = "", header = T)`` as a pandas DataFrame."""
    import pandas as pd
    return pd.read_csv(annotated_links_path, sep="\t", header=0, quoting=csv.QUOTE_NONE)


def _fmt_pos(x) -> str:
    x = float(x)
    return str(int(x)) if x.is_integer() else rcompat.format_number(x)


def _int_lines(pos) -> str:
    return "".join(f"{int(p)}\n" for p in np.asarray(pos).tolist())


def _match_positions(POS, pos):
    """(0-based SNP index of every value of ``pos``, the first value that matches no SNP or more than one, or None)."""
    P = np.asarray(POS, dtype=np.float64).ravel()
    p = np.asarray(pos, dtype=np.float64).ravel()
    order = np.argsort(P, kind="stable")
    srt = P[order]
    lo, hi = np.searchsorted(srt, p, side="left"), np.searchsorted(srt, p, side="right")
    bad = np.flatnonzero(hi - lo != 1)
    if len(bad):
        return None, p[bad[0]]
    return order[lo].astype(np.int32), None


def _select(POS, pos):
    """snpdat_to_fa's selection (R/io_functions.R:374-388): (SNP rows, positions in output order)."""
    if pos is None:
        return np.arange(len(POS), dtype=np.int32), np.asarray(POS)
    p = np.sort(np.asarray(pos, dtype=np.float64).ravel())
    if len(p) == 0:
        raise ValueError("pos is empty: there is no SNP to write")
    if np.any(p[1:] == p[:-1]):
        raise ValueError("Duplicated entries found in pos")
    idx, bad = _match_positions(POS, p)
    if idx is None:
        raise ValueError(f"pos= {_fmt_pos(bad)} cannot be extracted from snp.dat")
    return idx, p


def _check_alignment(snp_dat: SnpDat, engine, alignment_resident: bool):
    """The sequence names, checked against the alignment's shape: the engine's when it holds the alignment, ``snp_dat.states``' otherwise."""
    if alignment_resident:
        if engine is None:
            raise ValueError("alignment_resident=True needs the engine that holds the alignment")
        n_snp, n_seq = engine.L, engine.N
    else:
        if snp_dat.states is None:
            raise ValueError("snp_dat.states is None (the alignment stayed on the device): pass its engine with alignment_resident=True")
        n_snp, n_seq = int(snp_dat.states.shape[0]), int(snp_dat.states.shape[1])
    if n_snp != len(snp_dat.POS):
        raise ValueError(f"snp_dat.POS has {len(snp_dat.POS)} entries, the alignment {n_snp} SNPs")
    names = [str(x) for x in snp_dat.seq_names]
    if len(names) != n_seq:
        raise ValueError(f"snp_dat.seq_names has {len(names)} entries, the alignment {n_seq} sequences")
    if any("\n" in x for x in names):
        raise ValueError("a sequence name holds a newline")
    return names


def _write(snp_dat, path, idx, names, fmt: int, append: bool, engine, alignment_resident: bool) -> int:
    own = engine is None
    eng = engine or Engine(0)
    try:
        if not alignment_resident:
            eng.set_alignment(snp_dat.states)
        return eng.write_alignment(path, idx, names, format=fmt, append=append)
    finally:
        if own:
            eng.close()


def snpdat_to_fa(snp_dat: SnpDat, aln_path, pos_path=None, pos=None, format="fasta", *, engine: Engine | None = None,
                 alignment_resident: bool = False) -> None:
    """Mirror of ``snpdat_to_fa``: the SNPs at ``pos`` (all of them in index order when None) as a FASTA file APPENDED to ``aln_path`` plus
    the positions in ``pos_path`` (overwritten, one integer per line), or as the tsv of ``write.table(fasta, sep = "\\t", quote = F)``
    (overwritten: a header of the positions with no leading field, then one row per sequence)."""
    if format != "fasta" and format != "tsv":
        warnings.warn(f"Format {format} unsupported, has to be: <fasta> or <tsv>. Changed to default <fasta>", UserWarning, stacklevel=2)
        format = "fasta"
    if format == "fasta" and pos_path is None:
        raise ValueError("Saving in fasta format requires a path for the pos file <pos_path>")
    idx, pos_out = _select(snp_dat.POS, pos)
    names = _check_alignment(snp_dat, engine, alignment_resident)
    if format == "fasta":
        _write(snp_dat, aln_path, idx, names, 0, True, engine, alignment_resident)
        with open(pos_path, "w") as fh:
            fh.write(_int_lines(pos_out))
    else:
        with open(aln_path, "w") as fh:
            fh.write("\t".join(str(int(p)) for p in np.asarray(pos_out).tolist()) + "\n")
        _write(snp_dat, aln_path, idx, names, 1, True, engine, alignment_resident)


def generate_Links_SNPS_fasta(snp_dat: SnpDat, aln_path, pos_path, lr_tophits_path=None, lr_annotated_links_path=None, sr_tophits_path=None,
                              sr_annotated_links_path=None, *, engine: Engine | None = None, alignment_resident: bool = False) -> None:
    """Mirror of ``generate_Links_SNPS_fasta``: the FASTA (appended) and positions file of every SNP named in pos1 / pos2 of the given
    tophits and annotated-links files (sorted, without repeats)."""
    if lr_tophits_path is None and lr_annotated_links_path is None and sr_tophits_path is None and sr_annotated_links_path is None:
        raise ValueError("At least one links file must be provided")
    pos = []
    for path, reader in ((lr_tophits_path, read_TopHits), (sr_tophits_path, read_TopHits), (lr_annotated_links_path, read_AnnotatedLinks),
                         (sr_annotated_links_path, read_AnnotatedLinks)):
        if path is not None:
            t = reader(os.path.realpath(path))
            for col in ("pos1", "pos2"):
                if col not in t.columns:
                    raise ValueError(f"{path} has no {col} column")
            pos += [t["pos1"].to_numpy(dtype=np.float64), t["pos2"].to_numpy(dtype=np.float64)]
    pos = np.unique(np.concatenate(pos))
    snpdat_to_fa(snp_dat, aln_path, pos_path, pos=pos, format="fasta", engine=engine, alignment_resident=alignment_resident)


def outliers_table(tophits, links_type: str = "SR") -> str:
    """The text of ``snps.outliers``: ``write.table(outliers, quote = F, col.names = T, row.names = F)`` of the six columns as.numeric
    (R's 15-significant-digit rule: 100000 -> 1e+05, TRUE -> 1), space-separated, rows in tophits order.  SR: MI = srp and MI_wogaps = MI;
    a frame without srp (what ``perform_MI_computation`` returns, before SnpEff) gives srp_max.  LR: both are MI."""
    if links_type not in ("SR", "LR"):
        raise ValueError(f"links_type must be 'SR' or 'LR', not {links_type!r}")
    if tophits is None or len(tophits) == 0:
        raise ValueError("tophits is empty: there is no link to write")
    mi_col = "MI"
    if links_type == "SR":
        mi_col = "srp" if "srp" in tophits.columns else "srp_max"
    src = ("pos1", "pos2", "len", "ARACNE", mi_col, "MI")
    for col in src:
        if col not in tophits.columns:
            raise ValueError(f"tophits has no {col} column" + (" (nor srp)" if col == "srp_max" else ""))
    cols = [np.asarray(tophits[c], dtype=np.float64) for c in src]
    lines = [" ".join(OUTLIER_COLS) + "\n"]
    for row in zip(*(c.tolist() for c in cols)):
        lines.append(" ".join(rcompat.format_number(v) for v in row) + "\n")
    return "".join(lines)


def write_output_for_gwes_explorer(snp_dat: SnpDat, tophits, gwes_explorer_folder, links_type: str = "SR", *, engine: Engine | None = None,
                                   alignment_resident: bool = False) -> None:
    """Mirror of ``write_output_for_gwes_explorer``: ``snps.loci`` (the sorted positions of pos1 and pos2, one per line), ``snps.aln`` (their
    FASTA, from the device) and ``snps.outliers`` (``outliers_table``) in ``gwes_explorer_folder``, each file replaced.  No ``mega_dset``
    refusal: the alignment is streamed."""
    outliers = outliers_table(tophits, links_type)
    loci = np.unique(np.concatenate([np.asarray(tophits["pos1"], dtype=np.float64), np.asarray(tophits["pos2"], dtype=np.float64)]))
    idx, bad = _match_positions(snp_dat.POS, loci)
    if idx is None:
        raise ValueError(f"tophits position {_fmt_pos(bad)} does not belong to exactly one SNP of snp_dat")
    names = _check_alignment(snp_dat, engine, alignment_resident)
    os.makedirs(gwes_explorer_folder, exist_ok=True)
    paths = [os.path.join(gwes_explorer_folder, f) for f in ("snps.loci", "snps.aln", "snps.outliers")]
    for p in paths:
        if os.path.exists(p):
            os.unlink(p)
    with open(paths[0], "w") as fh:
        fh.write(_int_lines(loci))
    _write(snp_dat, paths[1], idx, names, 0, False, engine, alignment_resident)
    with open(paths[2], "w") as fh:
        fh.write(outliers)
