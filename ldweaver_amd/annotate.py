"""Mirror of ``perform_snpEff_annotations`` (R/SnpEffAnnotations.R:29-103): the SNPs of the links as ``<lr|sr>_snps.vcf``, a per-SNP
annotation table, the annotation joined onto every link and the top hits.

Two routes give the per-SNP table.  ``annotator="vcf"`` reads a snpEff-annotated VCF made elsewhere with ``convert_vcfann_to_table``'s
semantics (``read.table(quote = "")`` with R's ``type.convert``, the ``ANN`` fields split by R's ``strsplit`` rules).  ``annotator="native"``
(the default) predicts the first ``ANN`` entry from the CDS table, the reference and codon table 11 on the device (``Engine.annot_snps``,
k_annot_snp in csrc/ldw_annot.hip) and renders it in snpEff's vocabulary; the rule table is DESIGN.md 19, and it is not claimed to match
snpEff byte for byte.  No route starts Java or any other program: ``snpeff_jar`` is accepted and never executed.

Both routes share the join and selection on the device (``Engine.annot_map`` / ``Engine.annot_links``: positions to rows, R's stable
decreasing ``order``, ``detect_top_hits``) and the writers: ``<t>_annotations.tsv`` in Python, ``<t>_links_annotated.tsv`` and
``<t>_tophits.tsv`` through the threaded native writer with a string-table column kind.  Every argument check runs before an engine is made.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import re
import urllib.parse

import numpy as np

from . import _lib as L
from . import rcompat
from .engine import Engine

# effect codes of k_annot_snp (index = code)
EFFECTS = (None, "start_lost", "stop_gained", "stop_lost", "missense_variant", "start_retained_variant", "synonymous_variant",
           "stop_retained_variant", "coding_sequence_variant", "upstream_gene_variant", "downstream_gene_variant", "intergenic_region")
E_START_LOST, E_STOP_GAINED, E_STOP_LOST, E_MISSENSE, E_START_RETAINED, E_SYNONYMOUS, E_STOP_RETAINED, E_CODING, E_UPSTREAM, E_DOWNSTREAM, \
    E_INTERGENIC = range(1, 12)
AA3 = {"A": "Ala", "R": "Arg", "N": "Asn", "D": "Asp", "C": "Cys", "Q": "Gln", "E": "Glu", "G": "Gly", "H": "His", "I": "Ile", "L": "Leu",
       "K": "Lys", "M": "Met", "F": "Phe", "P": "Pro", "S": "Ser", "T": "Thr", "W": "Trp", "Y": "Tyr", "V": "Val", "*": "*"}
CODES = ("sy", "ns", "ig")
PAIRS = tuple(f"{a}X{b}" for a in CODES for b in CODES)
ANN_COLS = ("pos", "REF", "ALT", "annotation", "description", "cds", "code", "allele_dist")
SR_COLS = ("pos1", "pos2", "len", "ARACNE", "MI", "srp", "pos1_ann", "pos2_ann", "pos1_genreg", "pos2_genreg", "links", "pos1_ad", "pos2_ad")
LR_COLS = ("pos1", "pos2", "len", "ARACNE", "MI", "pos1_ann", "pos2_ann", "pos1_genreg", "pos2_genreg", "links", "pos1_ad", "pos2_ad")
NA = None


# ---- R's text rules ------------------------------------------------------------------------------------------------------------------

def r_strsplit(x, sep: str = "|"):
    """``strsplit(x, sep, fixed)[[1]]``: a trailing empty piece is dropped, a leading one kept; "" gives no piece; NA gives NA."""
    if x is NA:
        return [NA]
    parts = x.split(sep)
    if parts and parts[-1] == "":
        parts.pop()
    return parts


def r_paste_unique(fields) -> str:
    """``paste(unique(fields), collapse = ":")`` with NA printed as "NA"."""
    seen = []
    for f in fields:
        if f not in seen:
            seen.append(f)
    return ":".join("NA" if f is NA else f for f in seen)


def code_of(annotation) -> str:
    """The ``code`` of convert_vcfann_to_table (R/SnpEffAnnotations.R:294-298): the later grep wins; NA matches nothing."""
    c = "ns"
    if annotation is NA:
        return c
    for pat, v in (("synonymous_variant", "sy"), ("stop_retained_variant", "sy"), ("downstream_gene_variant", "ig"), ("upstream_gene_variant", "ig")):
        if pat in annotation:
            c = v
    return c


_LOGICAL = {"T": "TRUE", "F": "FALSE", "TRUE": "TRUE", "FALSE": "FALSE", "true": "TRUE", "false": "FALSE", "True": "TRUE", "False": "FALSE"}
_INT_RE = re.compile(r"^[-+]?[0-9]+$")


def _is_double(s: str) -> bool:
    if s in ("Inf", "-Inf", "+Inf", "NaN", "NA"):
        return True
    try:
        float(s)
    except ValueError:
        return False
    return not s.lower().lstrip("+-").startswith(("inf", "nan"))


def type_convert(values):
    """``type.convert(values, as.is = TRUE)`` of one read.table column, returned as the strings ``write.table(quote = F)`` / ``as.character``
    give back (NA as None): logical (all of T F TRUE FALSE true false True False) prints TRUE / FALSE, integer as read, double by the
    15-significant-digit rule, character unchanged.  "NA" is NA in every kind."""
    vals = [v for v in values if v != "NA"]
    if all(v in _LOGICAL for v in vals):
        return [NA if v == "NA" else _LOGICAL[v] for v in values]
    if all(_INT_RE.match(v) and abs(int(v)) <= 2147483647 for v in vals):
        return [NA if v == "NA" else str(int(v)) for v in values]
    if all(_is_double(v) for v in vals):
        return [NA if v == "NA" else rcompat.format_number(float(v)) for v in values]
    return [NA if v == "NA" else v for v in values]


def read_table_noquote(path):
    """The whitespace-separated fields of every data line of ``read.table(path, quote = "")``: '#' starts a comment, blank lines are
    skipped; every row must have the first row's field count."""
    rows = []
    with open(path, "r", encoding="utf-8", errors="replace") as fh:
        for lineno, line in enumerate(fh, 1):
            line = line.split("#", 1)[0]
            f = line.split()
            if not f:
                continue
            if rows and len(f) != len(rows[0]):
                raise ValueError(f"{path}: line {lineno} did not have {len(rows[0])} elements")
            rows.append(f)
    return rows


def fmt_int_or_num(x) -> str:
    x = float(x)
    return str(int(x)) if x.is_integer() else rcompat.format_number(x)


# ---- the VCF --------------------------------------------------------------------------------------------------------------------------

def vcf_text(genome_name: str, g, pos, ref, alt) -> str:
    """``append_vcf_header`` + ``create_vcf_file`` (R/SnpEffAnnotations.R:217-235): the header lines, then one row per SNP (POS by
    sprintf("%.0f"))."""
    lines = ["##fileformat=VCF4.1\n", f"##contig=<ID=1,length={fmt_int_or_num(g)}>\n",
             '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n', "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"]
    for p, r, a in zip(np.asarray(pos, dtype=np.float64).tolist(), ref, alt):
        lines.append(f"{genome_name}\t{'%.0f' % p}\t.\t{r}\t{a}\t.\t.\t.\n")
    return "".join(lines)


def genome_name_of(gbk=None, gff=None) -> str:
    """``gbk@genes@seqinfo@genome`` (the first word of VERSION, or "unknown": R/parseGBK.R:901-906) or ``gff$gff$seqid[1]``."""
    if gbk is not None:
        v = (getattr(gbk, "version", "") or "").split()
        return v[0] if v else "unknown"
    return str(gff.gff["seqid"].iloc[0]) if len(gff.gff) else "unknown"


def r_shquote(s) -> str:
    return "'" + str(s).replace("'", "'\\''") + "'"


def snpeff_command(dset_name, snpeff_jar, annotation_folder, vcf_path, ann_path) -> str:
    """The command line ``run_snpeff`` would run (R/SnpEffAnnotations.R:255-259); printed, never executed."""
    return " ".join(["java -Xmx16G -jar", r_shquote(snpeff_jar), "-v -dataDir", r_shquote(os.path.join(annotation_folder, "snpEff_data")),
                     "-config", r_shquote(os.path.join(annotation_folder, "snpEff.config")), r_shquote(dset_name), r_shquote(vcf_path), ">",
                     r_shquote(ann_path)])


# ---- the per-SNP table ----------------------------------------------------------------------------------------------------------------

def allele_dist(allele_table, snp_idx, nseq) -> list:
    """``getAlleleDistribution`` (R/SnpEffAnnotations.R:313-322): per SNP the non-zero A C G T N counts, decreasing (ties keep A C G T N
    order: R's radix sort is stable), as ``name:count/nseq`` joined by ", "."""
    at = np.asarray(allele_table)
    names = ("A", "C", "G", "T", "N")
    out = []
    for j in np.asarray(snp_idx).tolist():
        col = at[:, j].tolist()
        order = sorted((x for x in range(5) if col[x] > 0), key=lambda x: -col[x])
        out.append(", ".join(f"{names[x]}:{rcompat.format_number(col[x] / nseq)}" for x in order))
    return out


def vcfann_table(path):
    """``convert_vcfann_to_table``'s columns of an annotated VCF (R/SnpEffAnnotations.R:272-303): dict of lists pos, REF, ALT, annotation,
    description, cds, code (strings as R prints them, NA as None)."""
    rows = read_table_noquote(path)
    if not rows:
        raise ValueError(f"{path} holds no data line")
    if len(rows[0]) < 8:
        raise ValueError(f"{path}: a VCF data line has at least 8 fields, found {len(rows[0])}")
    cols = {name: type_convert([r[k] for r in rows]) for name, k in (("pos", 1), ("REF", 3), ("ALT", 4), ("ANN", 7))}
    ann = [NA if a is NA else a.replace('"', "") for a in cols["ANN"]]
    out = {"pos": cols["pos"], "REF": cols["REF"], "ALT": cols["ALT"], "annotation": [], "description": [], "cds": [], "code": []}
    for a in ann:
        f = r_strsplit(a)
        get = (lambda k: f[k - 1] if k <= len(f) else NA)
        out["annotation"].append(get(2))
        out["description"].append(r_paste_unique([get(4), get(5), get(10), get(11)]))
        out["cds"].append(get(5))
        out["code"].append(code_of(get(2)))
    return out


# ---- the features of the native route --------------------------------------------------------------------------------------------------

def _attrs(s: str) -> dict:
    d = {}
    for kv in str(s).split(";"):
        if "=" in kv:
            k, v = kv.split("=", 1)
            d.setdefault(k.strip(), urllib.parse.unquote(v.strip()))
    return d


def features_of(gbk=None, gff=None) -> dict:
    """The CDS features of the native route: ``seg`` (nseg x 3: lo, hi, feature; each feature's segments contiguous, in coding order),
    ``strand`` (+1 / -1), ``gene_id``, ``gene_name`` per feature in file order."""
    groups, keys = [], {}
    if gbk is not None:
        cds = gbk.cds
        st, en = np.asarray(cds["start"], dtype=np.int64), np.asarray(cds["end"], dtype=np.int64)
        sd = np.asarray(cds["strand"]).astype(str)
        feat = getattr(gbk, "feature", None)
        fid = np.arange(len(st)) if feat is None else np.asarray(feat)
        lt, ge = np.asarray(cds["locus_tag"]).astype(str), np.asarray(cds["gene"]).astype(str)
        seqname = str(gbk.seqname)
        for i in range(len(st)):
            k = int(fid[i])
            if k not in keys:
                keys[k] = len(groups)
                groups.append(dict(rows=[], strand=-1 if sd[i] == "-" else 1, attrs=[], seqname=seqname))
            g = groups[keys[k]]
            g["rows"].append((int(st[i]), int(en[i])))
            g["attrs"].append({"locus_tag": lt[i], "gene": ge[i]})
    else:
        df = gff.gff
        typ = np.char.lower(np.asarray(df["type"]).astype(str))
        for i in np.flatnonzero(typ == "cds").tolist():
            row = df.iloc[i]
            a = _attrs(row["attributes"])
            k = a.get("ID", "")
            key = ("id", k) if k else ("row", i)
            if key not in keys:
                keys[key] = len(groups)
                groups.append(dict(rows=[], strand=-1 if str(row["strand"]) == "-" else 1, attrs=[], seqname=str(row["seqid"])))
            g = groups[keys[key]]
            g["rows"].append((int(row["start"]), int(row["end"])))
            g["attrs"].append(a)
    seg, strand, gid, gname = [], [], [], []
    for f, g in enumerate(groups):
        rows = sorted(g["rows"], key=lambda r: r[0], reverse=g["strand"] < 0)
        seg += [(lo, hi, f) for lo, hi in rows]
        strand.append(g["strand"])

        def first(*names):
            for n in names:
                for a in g["attrs"]:
                    v = a.get(n, "")
                    if v:
                        return v
            return ""
        lo, hi = min(r[0] for r in rows), max(r[1] for r in rows)
        i_ = first("locus_tag") if gbk is not None else first("locus_tag", "ID")
        i_ = i_ or f"{g['seqname']}:{lo}-{hi}"
        n_ = (first("gene") if gbk is not None else first("gene", "Name")) or i_
        gid.append(i_)
        gname.append(n_)
    return dict(seg=np.asarray(seg, dtype=np.int32).reshape(-1, 3), strand=np.asarray(strand, dtype=np.int8), gene_id=gid, gene_name=gname)


def render_record(r, feats, pos) -> tuple:
    """(annotation, Gene_Name, Gene_ID, HGVS.c, HGVS.p) of one k_annot_snp record."""
    e, f, rf, c, k = int(r[0]), int(r[2]), int(r[3]), int(r[4]), int(r[5])
    rb, ab, ra, aa = (chr(x) if x else "" for x in (int(r[6]), int(r[7]), int(r[8]), int(r[9])))
    if e == E_INTERGENIC:
        ln = feats["gene_name"][f] if f >= 0 else "CHR_START"
        li = feats["gene_id"][f] if f >= 0 else "CHR_START"
        rn = feats["gene_name"][rf] if rf >= 0 else "CHR_END"
        ri = feats["gene_id"][rf] if rf >= 0 else "CHR_END"
        hc = f"n.{pos}{rb}>{ab}" if ab else ""
        return EFFECTS[e], f"{ln}-{rn}", f"{li}-{ri}", hc, ""
    name, gid = feats["gene_name"][f], feats["gene_id"][f]
    if e in (E_UPSTREAM, E_DOWNSTREAM):
        hc = (f"c.-{c}{rb}>{ab}" if e == E_UPSTREAM else f"c.*{c}{rb}>{ab}") if ab else ""
        return EFFECTS[e], name, gid, hc, ""
    hc = f"c.{c}{rb}>{ab}" if ab else ""
    if e == E_CODING:
        hp = ""
    elif e == E_START_LOST:
        hp = "p.Met1?"
    elif e == E_START_RETAINED:
        hp = "p.Met1Met"
    elif e == E_STOP_LOST:
        hp = f"p.*{k}{AA3[aa]}ext*?"
    elif e == E_STOP_RETAINED:
        hp = f"p.*{k}*"
    elif e == E_STOP_GAINED:
        hp = f"p.{AA3[ra]}{k}*"
    else:   # missense, synonymous
        hp = f"p.{AA3[ra]}{k}{AA3[aa]}"
    return EFFECTS[e], name, gid, hc, hp


def native_table(rec, feats, pos) -> dict:
    """annotation, description, cds, code of every record (the three fields derived as convert_vcfann_to_table derives them)."""
    out = {"annotation": [], "description": [], "cds": [], "code": []}
    for r, p in zip(rec, np.asarray(pos).tolist()):
        a, n, i, hc, hp = render_record(r, feats, int(p))
        out["annotation"].append(a)
        out["description"].append(r_paste_unique([n, i, hc, hp]))
        out["cds"].append(i)
        out["code"].append(code_of(a))
    return out


# ---- the files ------------------------------------------------------------------------------------------------------------------------

def _cell(v) -> str:
    return "NA" if v is NA else v


def annotations_text(tab: dict) -> str:
    """``write.table(ann, quote = F, row.names = F, sep = '\\t', col.names = T)``."""
    lines = ["\t".join(ANN_COLS) + "\n"]
    for row in zip(*(tab[c] for c in ANN_COLS)):
        lines.append("\t".join(_cell(v) for v in row) + "\n")
    return "".join(lines)


def _blob(strings):
    enc = [s.encode("utf-8") for s in strings]
    offs = np.zeros(len(enc) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(b) for b in enc]) if enc else []
    return b"".join(enc), offs


def write_links_table(path, header, num_cols, str_cols, table) -> int:
    """One header line, then the rows through ldw_write_table_tsv_str: ``num_cols`` (name, kind, array) and ``str_cols`` (name, base,
    int32 indices) in ``header`` order; ``table`` the strings.  Returns the bytes of the rows."""
    with open(path, "w") as fh:
        fh.write("\t".join(header) + "\n")
    byname = {n: (k, a, 0) for n, k, a in num_cols}
    byname.update({n: (L.COL_STR, a, b) for n, b, a in str_cols})
    kinds = np.array([byname[h][0] for h in header], dtype=np.int32)
    arrs = [np.ascontiguousarray(byname[h][1]) for h in header]
    bases = np.array([byname[h][2] for h in header], dtype=np.int64)
    ptrs = (C.c_void_p * len(header))(*[a.ctypes.data for a in arrs])
    blob, offs = _blob(table)
    nbytes = C.c_int64(0)
    n = len(arrs[0])
    L.check(L.lib().ldw_write_table_tsv_str(os.fsencode(str(path)), 1, n, len(header), L.ptr(kinds), ptrs, L.ptr(bases), blob, L.ptr(offs),
                                            len(table), 0, C.byref(nbytes)))
    return int(nbytes.value)


# ---- the entry point ------------------------------------------------------------------------------------------------------------------

def _paths(annotation_folder, links_type, tophits_path):
    t = links_type.lower()
    d = {k: os.path.join(annotation_folder, f"{t}_{k}") for k in ("snps.vcf", "snps_ann.vcf", "annotations.tsv", "links_annotated.tsv")}
    d["tophits.tsv"] = tophits_path if tophits_path is not None else os.path.join(annotation_folder, f"{t}_tophits.tsv")
    return d


def _check(snp_dat, cds_var, links_df, gbk, gff, max_tophits, links_type, annotator):
    if (gbk is None) == (gff is None):
        raise ValueError("Provide either one of gbk or gff")
    if links_type not in ("LR", "SR"):
        raise ValueError("Links type must be LR or SR")
    if annotator not in ("native", "vcf"):
        raise ValueError(f"annotator must be 'native' or 'vcf', not {annotator!r}")
    if isinstance(max_tophits, bool) or not float(max_tophits).is_integer() or max_tophits < 0:
        raise ValueError(f"max_tophits must be a non-negative integer, not {max_tophits!r}")
    need = ("pos1", "pos2", "len", "ARACNE", "MI") + (("srp_max",) if links_type == "SR" else ())
    for col in need:
        if col not in links_df.columns:
            raise ValueError(f"links_df has no {col} column")
    if len(links_df) == 0:
        raise ValueError("links_df is empty: there is no link to annotate")
    nsnp = len(snp_dat.POS)
    if cds_var.ref is None or cds_var.alt is None or cds_var.allele_table is None:
        raise ValueError("cds_var has no ref / alt / allele_table: make it with estimate_variation_in_CDS")
    if len(cds_var.ref) != nsnp or len(cds_var.alt) != nsnp or np.asarray(cds_var.allele_table).shape != (5, nsnp):
        raise ValueError(f"cds_var does not describe the {nsnp} SNPs of snp_dat")
    if gbk is not None:
        from .gbk import GenBankRecord
        rec = gbk.get("gbk") if isinstance(gbk, dict) else gbk
        if not isinstance(rec, GenBankRecord):
            raise NotImplementedError("gbk must be what parse_genbank_file returns (or its GenBankRecord)")
        gbk = rec
    # every link position must be exactly one SNP (R's which() would return none or several and fail obscurely)
    POS = np.asarray(snp_dat.POS, dtype=np.float64)
    order = np.argsort(POS, kind="stable")
    srt = POS[order]
    used = np.zeros(nsnp, dtype=bool)
    for col in ("pos1", "pos2"):
        p = np.asarray(links_df[col], dtype=np.float64)
        lo, hi = np.searchsorted(srt, p, side="left"), np.searchsorted(srt, p, side="right")
        bad = np.flatnonzero(hi - lo != 1)
        if len(bad):
            v = p[bad[0]]
            what = "no SNP" if hi[bad[0]] == lo[bad[0]] else "several SNPs"
            raise ValueError(f"links_df {col} = {fmt_int_or_num(v) if math.isfinite(v) else v} matches {what} of snp_dat (row {int(bad[0]) + 1})")
        used[lo] = True
    snps = order[used].astype(np.int32)   # the sorted distinct link positions, as SNP indices
    return gbk, snps


def perform_snpEff_annotations(dset_name, annotation_folder, snpeff_jar, snp_dat, cds_var, links_df, gbk=None, gbk_path=None, gff=None,
                               tophits_path=None, max_tophits=250, links_type="SR", *, engine: Engine | None = None, annotator: str = "native",
                               annotated_vcf=None):
    """Mirror of ``perform_snpEff_annotations``: writes ``<t>_snps.vcf``, ``<t>_annotations.tsv``, ``<t>_links_annotated.tsv`` and
    ``<t>_tophits.tsv`` (t = sr / lr; tophits at ``tophits_path`` when given) in ``annotation_folder`` and returns the top-hits frame
    (columns of add_annotations_to_links; LR ARACNE as bool).  ``annotator="native"``: the device predictor; ``"vcf"``: read
    ``annotated_vcf`` (default ``<folder>/<t>_snps_ann.vcf``) made by snpEff from the VCF written here; FileNotFoundError naming the command
    line when it is missing.  ``snpeff_jar`` and ``gbk_path`` are accepted; nothing is executed."""
    import pandas as pd
    gbk, snps = _check(snp_dat, cds_var, links_df, gbk, gff, max_tophits, links_type, annotator)
    paths = _paths(annotation_folder, links_type, tophits_path)
    pos = np.asarray(snp_dat.POS)[snps]
    refc = [str(x) for x in np.asarray(cds_var.ref)[snps].tolist()]
    altc = [str(cds_var.alt[j]) for j in snps.tolist()]
    os.makedirs(annotation_folder, exist_ok=True)
    with open(paths["snps.vcf"], "w") as fh:
        fh.write(vcf_text(genome_name_of(gbk, gff), snp_dat.g if snp_dat.g is not None else (gbk.g if gbk is not None else gff.g), pos, refc, altc))
    nseq = snp_dat.nseq
    if annotator == "vcf":
        ann_path = annotated_vcf if annotated_vcf is not None else paths["snps_ann.vcf"]
        if not os.path.exists(ann_path):
            raise FileNotFoundError(f"{ann_path} not found.  The SNPs to annotate were written to {paths['snps.vcf']}; annotate them with "
                                    f"snpEff (the reference runs: {snpeff_command(dset_name, snpeff_jar, annotation_folder, paths['snps.vcf'], ann_path)}) "
                                    "and pass the result as annotated_vcf, or use annotator='native'")
        tab = vcfann_table(ann_path)
        if len(tab["pos"]) != len(snps):
            raise ValueError(f"{ann_path} has {len(tab['pos'])} data lines, {len(snps)} SNPs were written")
        # every annotation row: the first line of the annotated VCF at its position (which(ann$pos %in% pp))
        apos = np.array([np.nan if v is NA else float(v) for v in tab["pos"]])
        o = np.argsort(apos, kind="stable")
        at = np.searchsorted(apos[o], pos.astype(np.float64), side="left")
        ok = (at < len(o)) & (apos[o[np.minimum(at, len(o) - 1)]] == pos)
        if not ok.all():
            raise ValueError(f"{ann_path} has no line at position {int(pos[np.flatnonzero(~ok)[0]])}")
        row_of = o[at]
    else:
        tab = None
    own = engine is None
    eng = engine or Engine(0)
    try:
        if annotator == "native":
            feats = features_of(gbk, gff)
            ref = np.asarray(gbk.sequence if gbk is not None else gff.ref, dtype=np.uint8)
            mask = np.array([sum(1 << "ACGT".index(ch) for ch in a.split(",") if ch in "ACGT") for a in altc], dtype=np.uint8)
            rec = eng.annot_snps(ref, feats["seg"], feats["strand"], pos, mask)
            nt = native_table(rec, feats, pos)
            tab = {"pos": [str(int(p)) for p in pos.tolist()], "REF": type_convert(refc), "ALT": type_convert(altc), **nt}
            row_of = np.arange(len(snps))
        tab["allele_dist"] = allele_dist(cds_var.allele_table, snps, nseq)
        with open(paths["annotations.tsv"], "w") as fh:
            fh.write(annotations_text(tab))
        dsnp, bad = eng.annot_map(links_df["pos1"], links_df["pos2"], snp_dat.POS)
        if bad >= 0 or not np.array_equal(dsnp, snps):
            raise RuntimeError("ldw_annot_map disagrees with the host's position check")
        # per annotation row (distinct link position): code, gene-region id, strings
        desc = [tab["description"][j] for j in row_of.tolist()]
        cds = [tab["cds"][j] for j in row_of.tolist()]
        ad = [tab["allele_dist"][j] for j in row_of.tolist()]
        code = np.array([CODES.index(tab["code"][j]) for j in row_of.tolist()], dtype=np.int8)
        uniq = {}
        cds_id = np.array([-1 if s is NA else uniq.setdefault(s, len(uniq)) for s in cds], dtype=np.int32)
        sr = links_type == "SR"
        key = np.asarray(links_df["srp_max" if sr else "MI"], dtype=np.float64)
        aracne = np.asarray(links_df["ARACNE"], dtype=np.float64)
        perm, r1, r2, pair, top = eng.annot_links(key, aracne, code, cds_id, int(max_tophits))
    finally:
        if own:
            eng.close()
    R = len(snps)
    table = desc + [_cell(s) for s in cds] + ad + list(PAIRS) + ["FALSE", "TRUE"]
    cols = _frame_cols(links_df, sr, perm)

    def emit(path, rows):
        num = [("pos1", L.COL_INT64, cols["pos1"][rows]), ("pos2", L.COL_INT64, cols["pos2"][rows]),
               ("len", L.COL_DOUBLE, cols["len"][rows]), ("MI", L.COL_DOUBLE, cols["MI"][rows])]
        strs = [("pos1_ann", 0, r1[rows]), ("pos2_ann", 0, r2[rows]), ("pos1_genreg", R, r1[rows]), ("pos2_genreg", R, r2[rows]),
                ("pos1_ad", 2 * R, r1[rows]), ("pos2_ad", 2 * R, r2[rows]), ("links", 3 * R, pair[rows].astype(np.int32))]
        if sr:
            num += [("ARACNE", L.COL_DOUBLE, cols["ARACNE"][rows]), ("srp", L.COL_DOUBLE, cols["srp"][rows])]
        else:
            strs.append(("ARACNE", 3 * R + 9, (cols["ARACNE"][rows] != 0).astype(np.int32)))
        return write_links_table(path, SR_COLS if sr else LR_COLS, num, [(n, b, np.ascontiguousarray(a, dtype=np.int32)) for n, b, a in strs], table)

    emit(paths["links_annotated.tsv"], slice(None))
    emit(paths["tophits.tsv"], top)
    out = {"pos1": cols["pos1"][top], "pos2": cols["pos2"][top], "len": cols["len"][top],
           "ARACNE": cols["ARACNE"][top] if sr else cols["ARACNE"][top] != 0, "MI": cols["MI"][top]}
    if sr:
        out["srp"] = cols["srp"][top]
    rr1, rr2 = r1[top], r2[top]
    out.update(pos1_ann=[desc[j] for j in rr1], pos2_ann=[desc[j] for j in rr2], pos1_genreg=[cds[j] for j in rr1],
               pos2_genreg=[cds[j] for j in rr2], links=[PAIRS[x] for x in pair[top]], pos1_ad=[ad[j] for j in rr1], pos2_ad=[ad[j] for j in rr2])
    return pd.DataFrame({c: out[c] for c in (SR_COLS if sr else LR_COLS)})


def _frame_cols(links_df, sr: bool, perm) -> dict:
    """The numeric columns of the annotated-links frame in sorted order (positions as integers: DESIGN.md 18)."""
    g = {"pos1": np.asarray(links_df["pos1"], dtype=np.float64)[perm].astype(np.int64),
         "pos2": np.asarray(links_df["pos2"], dtype=np.float64)[perm].astype(np.int64),
         "len": np.asarray(links_df["len"], dtype=np.float64)[perm], "ARACNE": np.asarray(links_df["ARACNE"], dtype=np.float64)[perm],
         "MI": np.asarray(links_df["MI"], dtype=np.float64)[perm]}
    if sr:
        g["srp"] = np.asarray(links_df["srp_max"], dtype=np.float64)[perm]
    return g
