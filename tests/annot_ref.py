"""Plain-Python restatement of the reference's SnpEff step (R/SnpEffAnnotations.R) and of the native rule table, written
apart from ldweaver_amd/annotate.py so that the tests hold the package against a second statement: append_vcf_header / create_vcf_file,
convert_vcfann_to_table (read.table(quote = "") with type.convert), getAlleleDistribution, add_annotations_to_links (the per-link loop),
detect_top_hits, and the effect of one SNP on one spliced feature, one codon at a time with a table-11 dictionary of its own.
"""
from __future__ import annotations

import math

from ldweaver_amd import rcompat

# ---- codon table 11 ---------------------------------------------------------------------------------------------------------------------
_B = "TCAG"
_AAS = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
TABLE11 = {a + b + c: _AAS[16 * i + 4 * j + k] for i, a in enumerate(_B) for j, b in enumerate(_B) for k, c in enumerate(_B)}
STARTS11 = {"ATG", "GTG", "TTG", "CTG", "ATT", "ATC", "ATA"}
THREE = dict(A="Ala", R="Arg", N="Asn", D="Asp", C="Cys", Q="Gln", E="Glu", G="Gly", H="His", I="Ile", L="Leu", K="Lys", M="Met", F="Phe",
             P="Pro", S="Ser", T="Thr", W="Trp", Y="Tyr", V="Val")
THREE["*"] = "*"
IMPACT = {"start_lost": 3, "stop_gained": 3, "stop_lost": 3, "missense_variant": 2, "start_retained_variant": 1, "synonymous_variant": 1,
          "stop_retained_variant": 1, "coding_sequence_variant": 0}
COMP = {"A": "T", "T": "A", "C": "G", "G": "C"}


def revcomp(s: str) -> str:
    return "".join(COMP.get(ch, ch) for ch in reversed(s))


# ---- R pieces ----------------------------------------------------------------------------------------------------------------------------

def r_num(x) -> str:
    return rcompat.format_number(x)


def r_pos(x) -> str:
    x = float(x)
    return str(int(x)) if x == int(x) else r_num(x)


def strsplit_bar(s):
    if s is None:
        return [None]
    out = s.split("|")
    if out and out[-1] == "":
        out = out[:-1]
    return out


def nth(fields, k):
    return fields[k - 1] if k <= len(fields) else None


def paste_unique(xs):
    u = []
    for x in xs:
        if x not in u:
            u.append(x)
    return ":".join("NA" if x is None else x for x in u)


def grep_code(a):
    code = "ns"
    if a is not None and "synonymous_variant" in a:
        code = "sy"
    if a is not None and "stop_retained_variant" in a:
        code = "sy"
    if a is not None and "downstream_gene_variant" in a:
        code = "ig"
    if a is not None and "upstream_gene_variant" in a:
        code = "ig"
    return code


def type_convert_col(col):
    """R's type.convert(as.is = TRUE) of one column, returned as printed strings (None = NA)."""
    lg = {"T": "TRUE", "TRUE": "TRUE", "true": "TRUE", "True": "TRUE", "F": "FALSE", "FALSE": "FALSE", "false": "FALSE", "False": "FALSE"}
    live = [x for x in col if x != "NA"]
    if all(x in lg for x in live):
        return [None if x == "NA" else lg[x] for x in col]

    def is_int(x):
        s = x[1:] if x[:1] in "+-" else x
        return s.isdigit() and abs(int(x)) < 2 ** 31

    if all(is_int(x) for x in live):
        return [None if x == "NA" else str(int(x)) for x in col]

    def is_num(x):
        if x in ("Inf", "-Inf", "NaN"):
            return True
        try:
            float(x)
            return x.lower().lstrip("+-")[:3] not in ("inf", "nan")
        except ValueError:
            return False

    if all(is_num(x) for x in live):
        return [None if x == "NA" else r_num(float(x)) for x in col]
    return [None if x == "NA" else x for x in col]


# ---- the reference's functions ------------------------------------------------------------------------------------------------------------

def vcf_file(genome_name, g, snps, REF, ALT) -> str:
    """append_vcf_header + create_vcf_file."""
    s = "##fileformat=VCF4.1\n" + "##contig=<ID=1,length=" + r_pos(g) + ">\n"
    s += "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n" + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
    for p, r, a in zip(snps, REF, ALT):
        s += "\t".join([genome_name, "%.0f" % float(p), ".", r, a, ".", ".", "."]) + "\n"
    return s


def allele_distribution(allele_table, idx, nseq):
    out = []
    for j in idx:
        col = [(n, int(allele_table[x][j])) for x, n in enumerate("ACGTN") if allele_table[x][j] > 0]
        col.sort(key=lambda t: -t[1])      # stable
        out.append(", ".join(f"{n}:{r_num(c / nseq)}" for n, c in col))
    return out


def convert_vcfann_to_table(text: str, snps_to_ann_idx, allele_table, nseq):
    """The ann data.frame as a list of row dicts (strings as write.table prints them, None = NA)."""
    rows = []
    for line in text.splitlines():
        line = line.split("#")[0]
        if line.strip():
            rows.append(line.split())
    cols = [type_convert_col([r[k] for r in rows]) for k in (1, 3, 4, 7)]
    ann = []
    for i in range(len(rows)):
        a = cols[3][i]
        a = None if a is None else a.replace('"', "")
        f = strsplit_bar(a)
        ann.append(dict(pos=cols[0][i], REF=cols[1][i], ALT=cols[2][i], annotation=nth(f, 2),
                        description=paste_unique([nth(f, 4), nth(f, 5), nth(f, 10), nth(f, 11)]), cds=nth(f, 5), code=grep_code(nth(f, 2))))
    for r, ad in zip(ann, allele_distribution(allele_table, snps_to_ann_idx, nseq)):
        r["allele_dist"] = ad
    return ann


def ann_tsv(ann) -> str:
    cols = ["pos", "REF", "ALT", "annotation", "description", "cds", "code", "allele_dist"]
    return "\t".join(cols) + "\n" + "".join("\t".join("NA" if r[c] is None else r[c] for c in cols) + "\n" for r in ann)


def add_annotations_to_links(links, ann, links_type="SR"):
    """links: dict of lists pos1 pos2 len ARACNE MI [srp_max]; returns the sorted l1_a1_d as a list of row dicts."""
    apos = [float(r["pos"]) for r in ann]
    n = len(links["pos1"])
    rows = []
    for i in range(n):
        i1 = apos.index(float(links["pos1"][i]))
        i2 = apos.index(float(links["pos2"][i]))
        r = dict(pos1=links["pos1"][i], pos2=links["pos2"][i], len=links["len"][i], ARACNE=links["ARACNE"][i], MI=links["MI"][i])
        if links_type == "SR":
            r["srp"] = links["srp_max"][i]
        r.update(pos1_ann=ann[i1]["description"], pos2_ann=ann[i2]["description"], pos1_genreg=ann[i1]["cds"], pos2_genreg=ann[i2]["cds"],
                 links=ann[i1]["code"] + "X" + ann[i2]["code"], pos1_ad=ann[i1]["allele_dist"], pos2_ad=ann[i2]["allele_dist"])
        rows.append(r)
    k = "srp" if links_type == "SR" else "MI"
    idx = sorted(range(n), key=lambda j: (math.isnan(rows[j][k]), -rows[j][k] if not math.isnan(rows[j][k]) else 0.0))
    return [rows[j] for j in idx]


def detect_top_hits(rows, max_tophits):
    a = [r for r in rows if r["ARACNE"] == 1]
    a = [r for r in a if r["links"] != "syXsy"]
    a = [r for r in a if r["pos1_genreg"] is not None and r["pos2_genreg"] is not None and r["pos1_genreg"] != r["pos2_genreg"]]
    return a[:max_tophits]


def links_tsv(rows, links_type="SR") -> str:
    cols = ["pos1", "pos2", "len", "ARACNE", "MI"] + (["srp"] if links_type == "SR" else []) + \
           ["pos1_ann", "pos2_ann", "pos1_genreg", "pos2_genreg", "links", "pos1_ad", "pos2_ad"]
    out = ["\t".join(cols) + "\n"]
    for r in rows:
        cells = []
        for c in cols:
            v = r[c]
            if c in ("pos1", "pos2"):
                cells.append(str(int(float(v))))
            elif c == "ARACNE":
                cells.append(r_num(float(v)) if links_type == "SR" else ("TRUE" if v else "FALSE"))
            elif c in ("len", "MI", "srp"):
                cells.append(r_num(float(v)))
            else:
                cells.append("NA" if v is None else v)
        out.append("\t".join(cells) + "\n")
    return "".join(out)


# ---- the native rule table -------------------------------------------------------------------------------------------------------------

def feature(segs, strand, gene_id, gene_name, idx):
    """segs: [(lo, hi)] in any order."""
    segs = sorted(segs)
    return dict(segs=segs, strand=strand, id=gene_id, name=gene_name, idx=idx, lo=segs[0][0], hi=max(h for _, h in segs))


def coding_seq(ref: str, f) -> str:
    s = "".join(ref[lo - 1:hi] for lo, hi in f["segs"]).upper()
    return s if f["strand"] > 0 else revcomp(s)


def coding_pos(f, p):
    """1-based c of genome position p on feature f, or None when p is in no segment."""
    segs = f["segs"] if f["strand"] > 0 else list(reversed(f["segs"]))
    off = 0
    for lo, hi in segs:
        if lo <= p <= hi:
            return off + (p - lo + 1 if f["strand"] > 0 else hi - p + 1)
        off += hi - lo + 1
    return None


def codon_effect(ref, f, p, allele):
    """(annotation, HGVS.c, HGVS.p) of one allele on one covering feature."""
    cds = coding_seq(ref, f)
    c = coding_pos(f, p)
    k = (c - 1) // 3 + 1
    rb = ref[p - 1].upper()
    if f["strand"] < 0:
        rb, allele = COMP.get(rb, rb), COMP[allele]
    hc = f"c.{c}{rb}>{allele}"
    codon = cds[3 * (k - 1):3 * k]
    if len(codon) < 3:
        return "coding_sequence_variant", hc, ""
    alt = list(codon)
    alt[(c - 1) % 3] = allele
    alt = "".join(alt)
    if k == 1 and codon in STARTS11:
        return ("start_retained_variant", hc, "p.Met1Met") if alt in STARTS11 else ("start_lost", hc, "p.Met1?")
    if codon not in TABLE11 or alt not in TABLE11:
        return "coding_sequence_variant", hc, ""
    a, b = TABLE11[codon], TABLE11[alt]
    if a == b:
        return ("stop_retained_variant", hc, f"p.*{k}*") if a == "*" else ("synonymous_variant", hc, f"p.{THREE[a]}{k}{THREE[a]}")
    if b == "*":
        return "stop_gained", hc, f"p.{THREE[a]}{k}*"
    if a == "*":
        return "stop_lost", hc, f"p.*{k}{THREE[b]}ext*?"
    return "missense_variant", hc, f"p.{THREE[a]}{k}{THREE[b]}"


def native_annotation(ref: str, feats, p: int, alt: str):
    """(annotation, Gene_Name, Gene_ID, HGVS.c, HGVS.p) of the SNP at p with ALT alt (cds_var$alt)."""
    alleles = [a for a in "ACGT" if a in alt.split(",")]
    cover = sorted((f for f in feats if coding_pos(f, p) is not None), key=lambda f: (f["lo"], f["idx"]))
    if cover:
        best = None
        for ai, a in enumerate(alleles):
            for f in cover:
                e, hc, hp = codon_effect(ref, f, p, a)
                key = (-IMPACT[e], ai, f["lo"], f["idx"], coding_pos(f, p))
                if best is None or key < best[0]:
                    best = (key, (e, f["name"], f["id"], hc, hp))
        if best is None:
            f = cover[0]
            return "coding_sequence_variant", f["name"], f["id"], "", ""
        return best[1]
    rb = ref[p - 1].upper()
    a0 = alleles[0] if alleles else None
    cand = []
    for f in feats:
        if f["hi"] < p:
            d, up = p - f["hi"], f["strand"] < 0
        elif f["lo"] > p:
            d, up = f["lo"] - p, f["strand"] > 0
        else:
            continue
        cand.append((d, not up, f["lo"], f["idx"], f))
    near = [x for x in cand if x[0] <= 5000]
    if near:
        d, down, _, _, f = min(near, key=lambda x: x[:4])
        if a0 is None:
            hc = ""
        else:
            r_, a_ = (rb, a0) if f["strand"] > 0 else (COMP.get(rb, rb), COMP[a0])
            hc = f"c.*{d}{r_}>{a_}" if down else f"c.-{d}{r_}>{a_}"
        return ("downstream_gene_variant" if down else "upstream_gene_variant"), f["name"], f["id"], hc, ""
    left = [f for f in feats if f["hi"] < p]
    right = [f for f in feats if f["lo"] > p]
    lf = min(left, key=lambda f: (-f["hi"], f["lo"], f["idx"])) if left else None
    rf = min(right, key=lambda f: (f["lo"], f["idx"])) if right else None
    name = (lf["name"] if lf else "CHR_START") + "-" + (rf["name"] if rf else "CHR_END")
    gid = (lf["id"] if lf else "CHR_START") + "-" + (rf["id"] if rf else "CHR_END")
    return "intergenic_region", name, gid, (f"n.{p}{rb}>{a0}" if a0 else ""), ""


def native_ann_rows(ref, feats, pos, REF, ALT, allele_table, idx, nseq):
    """The ann rows the native route gives (REF / ALT as read back from the VCF by type.convert)."""
    rc, ac = type_convert_col(list(REF)), type_convert_col(list(ALT))
    rows = []
    for i, (p, alt) in enumerate(zip(pos, ALT)):
        a, n, g, hc, hp = native_annotation(ref, feats, int(p), alt)
        rows.append(dict(pos=str(int(p)), REF=rc[i], ALT=ac[i], annotation=a, description=paste_unique([n, g, hc, hp]), cds=g, code=grep_code(a)))
    for r, ad in zip(rows, allele_distribution(allele_table, idx, nseq)):
        r["allele_dist"] = ad
    return rows
