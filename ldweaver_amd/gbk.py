"""Mirror of ``parse_genbank_file`` (R/parseGBK.R:27-86): a single-record GenBank file (plain or gzip) read by the native parser
(csrc/ldw_gbk.cpp, ``ldw_gbk_probe`` / ``ldw_gbk_read``) into the CDS rows and the reference sequence that ``estimate_variation_in_CDS``
reads from ``gbk@cds`` and ``gbk@sequence`` (R/estimateCDSDiversity.R:39-47).  Grammar, rejections and the declared divergence: DESIGN.md 17.
"""
from __future__ import annotations

import ctypes as C
import os
import warnings
from dataclasses import dataclass

import numpy as np

from . import _lib as L


@dataclass
class GenBankRecord:
    """What ``parse_genbank_file(...)["gbk"]`` holds: ``cds`` one row per CDS segment in file order (columns seqnames, start, end, strand,
    type, locus_tag, gene, product; start / end int64, 1-based inclusive), ``sequence`` the reference as uint8 UPPER-CASE characters cut to
    the source feature's range, its name ``seqname`` and length ``g``, and the LOCUS name, first ACCESSION and VERSION of the record."""
    cds: object              # pandas.DataFrame
    sequence: np.ndarray
    seqname: str
    g: int
    locus: str = ""
    accession: str = ""
    version: str = ""
    gbk_path: str | None = None
    feature: np.ndarray | None = None   # int64 per cds row: its feature (rows of one join() / order() share it); None: every row its own


def read_genbank(gbk_path) -> GenBankRecord:
    """The native parse of ``gbk_path`` as a GenBankRecord; ValueError (the parser's message, naming the line) for what it rejects."""
    import pandas as pd
    if not os.path.exists(gbk_path):
        raise FileNotFoundError(f"Can't locate file {gbk_path}")
    lib = L.lib()
    path = os.fsencode(str(gbk_path))

    def call(rc):
        if rc == L.LDW_ERR_ARG:
            raise ValueError(lib.ldw_last_error().decode("utf-8", "replace"))
        L.check(rc)

    nr, nf, g, nm = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    call(lib.ldw_gbk_probe(path, C.byref(nr), C.byref(nf), C.byref(g), C.byref(nm)))
    n = nr.value
    start = np.empty(n, dtype=np.int64)
    end = np.empty(n, dtype=np.int64)
    strand = np.empty(n, dtype=np.int8)
    feat = np.empty(n, dtype=np.int64)
    seq = np.empty(g.value, dtype=np.uint8)
    meta = np.empty(max(nm.value, 1), dtype=np.uint8)
    call(lib.ldw_gbk_read(path, n, L.ptr(start), L.ptr(end), L.ptr(strand), L.ptr(feat), g.value, L.ptr(seq), nm.value, L.ptr(meta)))
    strs = meta[:nm.value].tobytes().decode("utf-8", "replace").split("\0")[:-1]
    seqname, locus, accession, version = strs[:4]
    tags = np.array(strs[4:], dtype=object).reshape(nf.value, 3)
    cds = pd.DataFrame({"seqnames": [seqname] * n, "start": start, "end": end, "strand": np.where(strand < 0, "-", "+").astype(object),
                        "type": ["CDS"] * n, "locus_tag": tags[feat, 0], "gene": tags[feat, 1], "product": tags[feat, 2]})
    return GenBankRecord(cds=cds, sequence=seq, seqname=seqname, g=int(g.value), locus=locus, accession=accession, version=version,
                         gbk_path=str(gbk_path), feature=feat)


def parse_genbank_file(gbk_path, g=None, length_check=True) -> dict:
    """Mirror of ``parse_genbank_file``: ``{"gbk": GenBankRecord, "ref_g": its sequence length}`` with the reference's checks
    (R/parseGBK.R:42-79): ``length_check`` needs ``g`` and stops on a mismatch; without it a mismatch, or ``g=None``, only warns."""
    if length_check and g is None:
        raise ValueError("g must be provided to perform length check!")
    rec = read_genbank(gbk_path)
    ref_g = rec.g
    if length_check:
        if ref_g != g:
            raise ValueError("Genbank reference sequence length mismatches with the fasta alignment!")
    elif g is not None:
        if ref_g != g:
            warnings.warn("Fasta length does not match the genbank reference sequence length!", UserWarning, stacklevel=2)
    else:
        warnings.warn("Similarity between the genbank reference and fasta sequences NOT checked, ignore if <pos> was provided...", UserWarning,
                      stacklevel=2)
    return {"gbk": rec, "ref_g": ref_g}
