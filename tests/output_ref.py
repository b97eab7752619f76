"""Literal host port of the reference's alignment writers, the yardstick of ldweaver_amd.output: snpdat_to_fa (R/io_functions.R:363-417),
generate_Links_SNPS_fasta (:432-460) and write_output_for_gwes_explorer (R/createGWESExplorerOutput.R:23-76).

The character matrix is built as the reference builds it (one letter of "ACGTN" per one-hot state, then transposed) and the files are
written line by line, one write.table call per line, with the declared divergence of DESIGN.md 18: positions print as integers."""
import os

import numpy as np
import pandas as pd

from ldweaver_amd import rcompat

_LUT = np.array(list("ACGTN"))


def _fasta_matrix(states, snps_idx):
    """fasta[k, N] filled from the five one-hot matrices, then t(fasta): [N, k] characters"""
    return _LUT[np.asarray(states)[np.asarray(snps_idx)]].T


def _write_line(path, text, append=True):
    with open(path, "a" if append else "w") as fh:   # write.table(x, path, quote = F, col.names = F, row.names = F, append = T)
        fh.write(text + "\n")


def snpdat_to_fa(states, POS, seq_names, aln_path, pos_path=None, pos=None, format="fasta"):
    if format != "fasta" and format != "tsv":
        format = "fasta"
    if format == "fasta" and pos_path is None:
        raise ValueError("Saving in fasta format requires a path for the pos file <pos_path>")
    POS = np.asarray(POS)
    snps_idx = []
    if pos is None:
        snps_idx = list(range(len(POS)))
        pos = POS
    else:
        pos = np.sort(np.asarray(pos))
        if len(pos) != len(set(pos.tolist())):
            raise ValueError("Duplicated entries found in pos")
        for i in range(len(pos)):
            idx = np.flatnonzero(np.isin(POS, pos[i]))
            if len(idx) != 1:
                raise ValueError(f"pos= {pos[i]} cannot be extracted from snp.dat")
            snps_idx.append(int(idx[0]))
    fasta = _fasta_matrix(states, snps_idx)
    if format == "fasta":
        for i in range(len(seq_names)):
            _write_line(aln_path, ">" + seq_names[i])
            _write_line(aln_path, "".join(fasta[i, :]))
        with open(pos_path, "w") as fh:
            for p in pos:
                fh.write(f"{int(p)}\n")
    else:   # write.table(fasta, aln_path, sep = "\t", quote = F): row and column names, the header without a leading field
        with open(aln_path, "w") as fh:
            fh.write("\t".join(str(int(p)) for p in pos) + "\n")
            for i in range(len(seq_names)):
                fh.write("\t".join([seq_names[i]] + list(fasta[i, :])) + "\n")


def generate_Links_SNPS_fasta(states, POS, seq_names, aln_path, pos_path, lr_tophits_path=None, lr_annotated_links_path=None,
                              sr_tophits_path=None, sr_annotated_links_path=None):
    paths = (lr_tophits_path, sr_tophits_path, lr_annotated_links_path, sr_annotated_links_path)
    if all(p is None for p in paths):
        raise ValueError("At least one links file must be provided")
    pos = []
    for p in paths:
        if p is not None:
            temp = pd.read_csv(p, sep="\t", header=0, quoting=3)
            pos += list(temp["pos1"]) + list(temp["pos2"])
    pos = sorted(pos)
    pos = [p for i, p in enumerate(pos) if p not in pos[:i]]
    snpdat_to_fa(states, POS, seq_names, aln_path, pos_path, pos=pos, format="fasta")


def write_output_for_gwes_explorer(states, POS, seq_names, tophits, gwes_explorer_folder, links_type="SR"):
    os.makedirs(gwes_explorer_folder, exist_ok=True)
    loci_pth = os.path.join(gwes_explorer_folder, "snps.loci")
    aln_pth = os.path.join(gwes_explorer_folder, "snps.aln")
    outliers_pth = os.path.join(gwes_explorer_folder, "snps.outliers")
    gwex_snps = sorted(set(list(tophits["pos1"]) + list(tophits["pos2"])))
    POS = np.asarray(POS)
    gwes_snps_idx = []
    for x in gwex_snps:
        idx = np.flatnonzero(np.isin(POS, x))
        assert len(idx) == 1
        gwes_snps_idx.append(int(idx[0]))
    if os.path.exists(loci_pth):
        os.unlink(loci_pth)
    with open(loci_pth, "w") as fh:
        for p in gwex_snps:
            fh.write(f"{int(p)}\n")
    fasta = _fasta_matrix(states, gwes_snps_idx)
    if os.path.exists(aln_pth):
        os.unlink(aln_pth)
    for i in range(len(seq_names)):
        _write_line(aln_pth, ">" + seq_names[i])
        _write_line(aln_pth, "".join(fasta[i, :]))
    mi = "MI"
    if links_type == "SR":
        mi = "srp" if "srp" in tophits.columns else "srp_max"
    outliers = pd.DataFrame({"Pos_1": np.asarray(tophits["pos1"], dtype=float), "Pos_2": np.asarray(tophits["pos2"], dtype=float),
                             "Distance": np.asarray(tophits["len"], dtype=float), "Direct": np.asarray(tophits["ARACNE"], dtype=float),
                             "MI": np.asarray(tophits[mi], dtype=float), "MI_wogaps": np.asarray(tophits["MI"], dtype=float)})
    if os.path.exists(outliers_pth):
        os.unlink(outliers_pth)
    with open(outliers_pth, "w") as fh:   # write.table(outliers, quote = F, col.names = T, row.names = F): sep " "
        fh.write(" ".join(outliers.columns) + "\n")
        for r in range(len(outliers)):
            fh.write(" ".join(rcompat.format_number(float(outliers.iloc[r, c])) for c in range(outliers.shape[1])) + "\n")
