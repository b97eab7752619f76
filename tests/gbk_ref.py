"""Restatement of the reference's GenBank parser (R/parseGBK.R: readGenBank2, parseGenBank, readFeatures, make_feat_gr, .do_join_silliness,
readOrigin, and the row stacking of fill_stack_df / make_cdsgr) for the tests of ldweaver_amd.gbk: a LITERAL port, statement by statement,
with R's regular expressions written for Python's re (POSIX classes spelled out).  It keeps what estimate_variation_in_CDS reads — the CDS
rows, the seqnames they carry, the sequence — and the qualifiers locus_tag, gene and product.  Where R stops with an error (an NA start,
a negative width, no sequence, several records, runaway recursion) the port raises RStop."""
from __future__ import annotations

import gzip
import re

SP = r"[ \t\n\r\f\v]"        # [[:space:]]
NSP = r"[^ \t\n\r\f\v]"      # [^[:space:]]
DNA_ALPHABET = set("ACGTMRWSYKVHDBN-+.")


class RStop(Exception):
    """An R error of the reference."""


def read_lines(data: bytes) -> list[str]:
    """readLines on a plain or gzip file: LF, CRLF and CR end a line; a last line without an end is kept."""
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)
    lines = re.split(r"\r\n|\r|\n", data.decode("latin-1"))
    if lines and lines[-1] == "":
        lines.pop()
    return lines


def r_strsplit(x: str, pattern: str) -> list[str]:
    """strsplit(x, pattern)[[1]]: no trailing empty piece."""
    out = re.split(pattern, x)
    if out and out[-1] == "":
        out.pop()
    return out


def as_integer(s: str):
    """as.integer() of a character value; None is NA."""
    s = s.strip(" \t\n\r\f\v")
    if re.fullmatch(r"[+-]?[0-9]+", s):
        return int(s)
    if re.fullmatch(r"[+-]?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][+-]?[0-9]+)?", s):
        return int(float(s))
    return None


# ---- R/parseGBK.R:407-412 -------------------------------------------------------------------------------------------------------------
def chk_outer_complement(s):
    return re.search(r"[^(]*complement\(", s) is not None


def strip_outer_operator(s, op="complement"):
    return re.sub(r"[^(]*" + op + r"\((.*)\)", r"\1", s)


# ---- :414-443 ---------------------------------------------------------------------------------------------------------------------------
def do_join_silliness(s, chr_, ats, strand=None):
    # the partial check (:417-431) never fires: '<' and '>' were deleted from the text (:133)
    sstr = s[:1]
    if sstr == "j":
        s = strip_outer_operator(s, "join")
    elif sstr == "o":
        s = strip_outer_operator(s, "order")
    spl = r_strsplit(s, ",")
    rows = []
    for x in spl:
        rows += make_feat_gr(x, chr_, ats, strand)
    return rows


# ---- :446-489 ---------------------------------------------------------------------------------------------------------------------------
def make_feat_gr(s, chr_, ats, strand=None):
    if strand is None and chk_outer_complement(s):
        strand = "-"
        s = strip_outer_operator(s)
    sbstr = s[:4]
    if sbstr == "join" or sbstr == "orde":
        return do_join_silliness(s, chr_, ats, strand)
    spl = r_strsplit(s, r"[.^]{1,2}")
    if not spl:
        raise RStop(f"no range in {s!r}")
    start = as_integer(re.sub(r"<*([0-9]+).*", r"\1", spl[0]))
    if len(spl) == 1:
        end = start
    else:
        end = as_integer(re.sub(r">*([0-9]+).*", r"\1", spl[1]))
    if "^" in s:
        end = None if end is None else end - 1
    if strand is None:
        strand = "+"
    return [{"seqnames": chr_, "start": start, "end": end, "strand": strand, **ats}]


# ---- :491-502 ---------------------------------------------------------------------------------------------------------------------------
def read_feat_attr(line):
    num = re.search(r"=[0-9]+(\.[0-9]+){0,1}$", line) is not None
    val = re.sub(SP + r'*/[^=]+($|="{0,1}([^"]*)"{0,1})', r"\2", line)
    if len(val) == 0:
        return True
    if num:
        return float(val)
    return val


def strip_feat_type(ln):
    return re.sub(r"^" + SP + r"*[A-Za-z0-9_'-]+" + SP + r"+((complement\(|join\(|order\(|[0-9<]+).*)", r"\1", ln)


# ---- :517-594 ---------------------------------------------------------------------------------------------------------------------------
def read_features(lines):
    sec_field_re = r"^( {5}|\t)[A-Za-z0-9'_-]+" + SP + r"+(complement|join|order|[0-9<,])"
    if lines[0][:8] == "FEATURES":
        lines = lines[1:]
    fttypelins = [re.search(sec_field_re, t) is not None for t in lines]
    groups = {}
    k = 0
    for t, f in zip(lines, fttypelins):
        k += f
        groups.setdefault(k, []).append(t)
    if 0 in groups:
        raise RStop("lines before the first feature")   # (the port does not follow what R makes of them)
    st = {"chr": "unk", "numsources": 0, "everhadchr": False}
    totsources = sum(1 for t, f in zip(lines, fttypelins) if f and re.search(SP + r"+source" + SP + r"+[<0-9]", t))

    def do_readfeat(lines):
        type_ = re.sub(SP + r"+([A-Za-z0-9_'-]+).*", r"\1", lines[0])
        attrstrts = []
        c = 0
        for t in lines:
            c += re.search(r"^" + SP + r"+/" + NSP + r'+($|=([0-9]|"))', t) is not None
            attrstrts.append(c)
        pieces = {}
        for t, a in zip(lines, attrstrts):
            pieces.setdefault(a, []).append(re.sub(r"^" + SP + r"+", "", t))
        pieces = ["".join(pieces[a]) for a in sorted(pieces)]
        rngstr = strip_feat_type(pieces[0])
        rest = pieces[1:]
        attrs = {}
        if rest:
            for ln in rest:
                nm = re.sub(r"^" + SP + r"*/([^=]+)($|=" + NSP + r".*$)", r"\1", ln)
                attrs.setdefault(nm, read_feat_attr(ln))      # attrs$name: the first of that name
            if type_ == "source":
                st["numsources"] += 1
                if "chromosome" in attrs:
                    if st["numsources"] > 1 and not st["everhadchr"]:
                        raise RStop("mixed chromosome names")
                    st["everhadchr"] = True
                    st["chr"] = attrs["chromosome"]
                elif st["everhadchr"]:
                    raise RStop("mixed chromosome names")
                elif "strain" in attrs:
                    st["chr"] = attrs["strain"] if totsources == 1 else f"{attrs['strain']}:{st['numsources']}"
                else:
                    st["chr"] = attrs.get("organism") if totsources == 1 else f"{attrs.get('organism')}:{st['numsources']}"
        return type_, make_feat_gr(rngstr, st["chr"], {"type": type_, "attrs": attrs})

    try:
        return [do_readfeat(groups[k]) for k in sorted(groups)]
    except RecursionError:
        raise RStop("infinite recursion (an unclosed join or order)") from None


# ---- :599-612 ---------------------------------------------------------------------------------------------------------------------------
def read_origin(lines):
    dnachar = [re.sub("(" + SP + "+|[0-9]+|//)", "", t) for t in lines[1:]]
    chars = "".join(dnachar)
    if any(len(x) for x in dnachar):
        bad = [c for c in chars if c.upper() not in DNA_ALPHABET]      # Biostrings::DNAString (upper-cases; checked against R: no)
        if bad:
            raise RStop(f"key {ord(bad[0])} (char '{bad[0]}') not in lookup table")
        return chars.upper()
    return None


# ---- readGenBank2 (:89-122), parseGenBank (:125-194), make_gbrecord (:196-262), parse_genbank_file (:50-63) --------------------------
def parse_genbank(lines):
    """{"rows": [(start, end, strand)], "feature": CDS feature index per row, "seqnames": per row, "tags": (locus_tag, gene, product) per
    CDS feature (R values: True for a bare flag), "sequence": str} of a CDS-bearing record, or RStop."""
    recbrks = [i for i, t in enumerate(lines) if re.search(r"^" + SP + r"*//" + SP + r"*$", t)]
    if len(recbrks) > 1:
        raise RStop(f"{len(recbrks)} records")
    text = [re.sub("[<>]", "", t) for t in lines]
    fldlines = [re.search(r"^[A-Z]", t) is not None for t in text]
    if not fldlines or not fldlines[0]:
        raise RStop("text before the first field")
    spl = {}
    name = None
    for t, f in zip(text, fldlines):
        if f:
            name = re.sub(r"^([A-Z]+).*", r"\1", t)
        spl.setdefault(name, []).append(t)
    if "LOCUS" not in spl:
        raise RStop("no LOCUS")
    if "FEATURES" not in spl:
        raise RStop("no FEATURES")
    feats = read_features(spl["FEATURES"])
    origin = read_origin(spl["ORIGIN"]) if "ORIGIN" in spl else None
    if origin is None:
        raise RStop("The GBK file should contain the reference sequence!")
    for _, rows in feats:          # every feature becomes a GRanges: IRanges(start, end) refuses NA and negative widths
        for r in rows:
            if r["start"] is None or r["end"] is None:
                raise RStop("NA start or end")
            if r["end"] < r["start"] - 1:
                raise RStop("negative width")
    srcs = [r for t, rows in feats if t == "source" for r in rows]
    if len(srcs) != 1:
        raise RStop("The GBK file should contain the reference sequence!")
    s0, e0 = srcs[0]["start"], srcs[0]["end"]
    if s0 < 1 or e0 > len(origin):
        raise RStop("extractAt: out of bounds")
    seqlevel = srcs[0]["seqnames"]
    out = {"rows": [], "feature": [], "seqnames": [], "tags": [], "sequence": origin[s0 - 1:e0]}
    k = 0
    for t, rows in feats:
        if t != "CDS":
            continue
        for r in rows:
            if r["seqnames"] != seqlevel:
                raise RStop("seqlevels not in seqinfo")
            out["rows"].append((r["start"], r["end"], r["strand"]))
            out["feature"].append(k)
            out["seqnames"].append(r["seqnames"])
        a = rows[0]["attrs"]
        out["tags"].append(tuple(a.get(q, "") for q in ("locus_tag", "gene", "product")))
        k += 1
    return out
