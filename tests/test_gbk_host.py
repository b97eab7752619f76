"""CPU: the native GenBank reader (csrc/ldw_gbk.cpp through ldweaver_amd.gbk) — every location form, multi-line locations and qualifiers,
tab-indented keys, CRLF / CR / gzip input, the ORIGIN rules, the source cut, every error and warning — and random files against the literal
port of the reference's parser (tests/gbk_ref.py), plus the parse time of a bacterial-scale file."""
import gzip
import time
import warnings

import numpy as np
import pytest

import gbk_ref as R
from ldweaver_amd import GenBankRecord, parse_genbank_file
from ldweaver_amd import cds
from ldweaver_amd.gbk import read_genbank

HEAD = ("LOCUS       TST0001                 {g} bp    DNA     circular BCT 01-JAN-2024\n"
        "DEFINITION  Testus syntheticus strain T1, complete genome.\n"
        "ACCESSION   TST0001\nVERSION     TST0001.1\nKEYWORDS    .\nSOURCE      Testus syntheticus\n"
        "  ORGANISM  Testus syntheticus\n            Bacteria; Testia.\n"
        "FEATURES             Location/Qualifiers\n")


def _origin(seq: str, width=60) -> str:
    out = ["ORIGIN      \n"]
    for i in range(0, len(seq), width):
        chunk = seq[i:i + width]
        out.append(f"{i + 1:>9} " + " ".join(chunk[j:j + 10] for j in range(0, len(chunk), 10)) + "\n")
    return "".join(out) + "//\n"


def _feature(key, loc, quals=(), tab=False):
    ind, qind = ("\t", "\t\t\t") if tab else (" " * 5, " " * 21)
    if isinstance(loc, str):
        loc = [loc]
    lines = [f"{ind}{key:<15} {loc[0]}" if not tab else f"{ind}{key}\t{loc[0]}"] + [qind + x for x in loc[1:]]
    for q in quals:
        q = [q] if isinstance(q, str) else list(q)
        lines += [qind + q[0]] + [qind + x for x in q[1:]]
    return "\n".join(lines) + "\n"


def _gbk(features, seq, source=None, src_quals=('/organism="Testus syntheticus"', '/strain="T1"'), tail="", head=HEAD):
    src = _feature("source", source or f"1..{len(seq)}", src_quals)
    return head.format(g=len(seq)) + src + "".join(features) + tail + _origin(seq)


def _write(tmp_path, text, name="a.gbk", eol="\n"):
    p = tmp_path / name
    data = text.replace("\n", eol).encode("latin-1")
    if name.endswith(".gz"):
        data = gzip.compress(data)
    p.write_bytes(data)
    return str(p)


def _rows(rec):
    c = rec.cds
    return list(zip(c["start"].tolist(), c["end"].tolist(), c["strand"].tolist()))


def _seq(n, seed=0):
    return "".join(np.random.default_rng(seed).choice(list("acgt"), size=n))


def _read(tmp_path, text, **kw):
    return _quiet(_write(tmp_path, text, **kw))


def _quiet(path):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return parse_genbank_file(path, length_check=False)["gbk"]


LOCATIONS = [
    ("100..200", [(100, 200, "+")]),
    ("150", [(150, 150, "+")]),
    ("150^151", [(150, 150, "+")]),                        # a^b -> [a, b - 1]
    ("120^125", [(120, 124, "+")]),
    ("complement(30..90)", [(30, 90, "-")]),
    ("join(10..20,30..40,5..8)", [(10, 20, "+"), (30, 40, "+"), (5, 8, "+")]),
    ("order(50..60,1..2,70)", [(50, 60, "+"), (1, 2, "+"), (70, 70, "+")]),
    ("complement(join(200..210,100..120))", [(200, 210, "-"), (100, 120, "-")]),
    ("complement(order(3..9,12^13))", [(3, 9, "-"), (12, 12, "-")]),
    ("<1..>40", [(1, 40, "+")]),                           # partial ends: '<' and '>' deleted, the CDS kept
    ("join(<5..10,20..>30)", [(5, 10, "+"), (20, 30, "+")]),
    ("complement(<250..>299)", [(250, 299, "-")]),
    ("60..59", [(60, 59, "+")]),                           # zero width is accepted, like IRanges
]


@pytest.mark.parametrize("loc,rows", LOCATIONS)
def test_location_forms(tmp_path, loc, rows):
    seq = _seq(300)
    rec = _read(tmp_path, _gbk([_feature("CDS", loc, ['/locus_tag="X_1"'])], seq))
    assert _rows(rec) == rows
    lit = R.parse_genbank(R.read_lines(open(tmp_path / "a.gbk", "rb").read()))
    assert lit["rows"] == rows
    assert rec.cds["locus_tag"].tolist() == ["X_1"] * len(rows) and rec.cds["type"].tolist() == ["CDS"] * len(rows)


def test_multiline_locations_and_qualifiers(tmp_path):
    seq = _seq(500, 1)
    feats = [
        _feature("gene", "10..90", ['/gene="abcD"']),
        _feature("CDS", ["complement(join(10..20,", "30..40,", "50..90))"],
                 ['/gene="abcD"', '/locus_tag="TST_0001"', ('/product="ABC transporter', 'permease subunit"'), "/codon_start=1",
                  ("/translation=\"MKVLAAGLLLLAVSAQAA", "MKKLLPTAAAGLLLLAAQPAMA\""), "/pseudo"]),
        _feature("misc_feature", "95..99", ['/note="a <note> with brackets"']),
        _feature("CDS", ["join(100..150,", "  160..199)"], ['/locus_tag="TST_0002"', '/product="hypothetical protein"']),
        _feature("tRNA", "complement(210..280)", ['/product="tRNA-Ala"']),
        _feature("CDS", "300..>410", ['/locus_tag="TST_0003"', ('/note="runs over', 'two lines"')]),
    ]
    rec = _read(tmp_path, _gbk(feats, seq))
    assert _rows(rec) == [(10, 20, "-"), (30, 40, "-"), (50, 90, "-"), (100, 150, "+"), (160, 199, "+"), (300, 410, "+")]
    c = rec.cds
    assert c["locus_tag"].tolist() == ["TST_0001"] * 3 + ["TST_0002"] * 2 + ["TST_0003"]
    assert c["gene"].tolist() == ["abcD"] * 3 + [""] * 3
    # continuation lines are joined without a separator after their leading blanks go, as paste(collapse = "") does (R/parseGBK.R:546-548)
    assert c["product"].tolist() == ["ABC transporterpermease subunit"] * 3 + ["hypothetical protein"] * 2 + [""]
    assert set(c["seqnames"]) == {"T1"} and rec.seqname == "T1"
    assert rec.locus == "TST0001" and rec.accession == "TST0001" and rec.version == "TST0001.1"
    assert rec.sequence.tobytes() == seq.upper().encode() and rec.g == 500 and rec.sequence.dtype == np.uint8
    lit = R.parse_genbank(R.read_lines(open(tmp_path / "a.gbk", "rb").read()))
    assert lit["rows"] == _rows(rec) and lit["sequence"] == seq.upper()
    assert [t[0] for t in lit["tags"]] == ["TST_0001", "TST_0002", "TST_0003"] and lit["tags"][0][2] == "ABC transporterpermease subunit"


@pytest.mark.parametrize("eol,name,tab", [("\n", "a.gbk", True), ("\r\n", "a.gbk", False), ("\r", "a.gbk", False), ("\r\n", "a.gbk.gz", True),
                                          ("\n", "a.gbk.gz", False)])
def test_line_endings_tabs_and_gzip(tmp_path, eol, name, tab):
    seq = _seq(240, 2)
    feats = [_feature("CDS", "complement(5..60)", ['/locus_tag="A_1"', ('/product="first', ' product"')], tab=tab),
             _feature("CDS", ["join(70..80,", "90..120)"], ['/locus_tag="A_2"'], tab=tab)]
    rec = _quiet(_write(tmp_path, _gbk(feats, seq), name=name, eol=eol))
    assert _rows(rec) == [(5, 60, "-"), (70, 80, "+"), (90, 120, "+")]
    assert rec.cds["locus_tag"].tolist() == ["A_1", "A_2", "A_2"] and rec.cds["product"][0] == "firstproduct"      # continuation joined after its blanks go
    assert rec.sequence.tobytes() == seq.upper().encode()


def test_origin_numbers_case_and_source_cut(tmp_path):
    seq = "acgtnRYKMswbdhv-+.ACGTacgt" * 4
    text = _gbk([_feature("CDS", "3..20")], seq, source="5..90")
    rec = _read(tmp_path, text)
    assert rec.g == 86 and rec.sequence.tobytes() == seq.upper()[4:90].encode()
    assert R.parse_genbank(R.read_lines(open(tmp_path / "a.gbk", "rb").read()))["sequence"] == seq.upper()[4:90]
    # line numbers, blanks and '//' go; a file without the final '//' reads the same
    rec2 = _read(tmp_path, text.replace("//\n", ""), name="b.gbk")
    assert rec2.sequence.tobytes() == rec.sequence.tobytes()


def test_length_checks_and_warnings(tmp_path):
    p = _write(tmp_path, _gbk([_feature("CDS", "3..20")], _seq(120, 3)))
    with pytest.raises(ValueError, match="g must be provided to perform length check!"):
        parse_genbank_file(p)
    with pytest.raises(ValueError, match="Genbank reference sequence length mismatches with the fasta alignment!"):
        parse_genbank_file(p, g=121)
    out = parse_genbank_file(p, g=120.0)
    assert out["ref_g"] == 120 and isinstance(out["gbk"], GenBankRecord) and out["gbk"].gbk_path == p
    with pytest.warns(UserWarning, match="Fasta length does not match the genbank reference sequence length!"):
        parse_genbank_file(p, g=7, length_check=False)
    with pytest.warns(UserWarning, match="Similarity between the genbank reference and fasta sequences NOT checked"):
        parse_genbank_file(p, length_check=False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        parse_genbank_file(p, g=120, length_check=False)
    with pytest.raises(FileNotFoundError):
        parse_genbank_file(str(tmp_path / "missing.gbk"), g=1)


NOSEQ = "The GBK file should contain the reference sequence!"


@pytest.mark.parametrize("case,match", [
    ("negative", r"line 13: a segment of negative width.*500\.\.400"),
    ("negative_join", r"line 13: a segment of negative width"),
    ("remote", r"line 13: a feature location outside the supported grammar.*J00194"),
    ("remote_join", r"line 13: a location outside the supported grammar.*J00194"),
    ("gap", r"line 13: a feature location outside the supported grammar.*gap\(\)"),
    ("one_of", r"line 13: a feature location outside the supported grammar.*one-of"),
    ("nested", r"line 13: join\(\) or order\(\) nested"),
    ("no_origin", NOSEQ),
    ("empty_origin", NOSEQ),
    ("no_source", NOSEQ),
    ("two_sources", NOSEQ),
    ("source_join", NOSEQ),
    ("two_records", r"holds 2 GenBank records"),
    ("bad_char", r"character 'j'.*not an IUPAC DNA letter"),
    ("cds_first", r"line 10: a CDS feature before the source feature"),
])
def test_errors(tmp_path, case, match):
    seq = _seq(600, 4)
    cds_ = {"negative": "500..400", "negative_join": "join(1..10,500..400)", "remote": "J00194.1:100..202",
            "remote_join": "join(1..10,J00194.1:100..202)", "gap": "gap()", "one_of": "one-of(1,2)..100", "nested": "join(1..2,join(3..4,5..6))"}
    if case in cds_:
        text = _gbk([_feature("CDS", cds_[case])], seq)
    elif case == "no_origin":
        text = _gbk([_feature("CDS", "1..10")], seq).split("ORIGIN")[0]
    elif case == "empty_origin":
        text = _gbk([_feature("CDS", "1..10")], seq).split("ORIGIN")[0] + "ORIGIN\n//\n"
    elif case == "no_source":
        text = HEAD.format(g=600) + _feature("CDS", "1..10") + _origin(seq)
    elif case == "two_sources":
        text = _gbk([_feature("source", "1..600", ['/organism="B"']), _feature("CDS", "1..10")], seq)
    elif case == "source_join":
        text = _gbk([_feature("CDS", "1..10")], seq, source="join(1..300,301..600)")
    elif case == "two_records":
        one = _gbk([_feature("CDS", "1..10")], seq)
        text = one + one
    elif case == "bad_char":
        text = _gbk([_feature("CDS", "1..10")], seq[:100] + "j" + seq[101:])
    elif case == "cds_first":
        text = HEAD.format(g=600) + _feature("CDS", "1..10") + _feature("source", "1..600", ['/organism="B"']) + _origin(seq)
    p = _write(tmp_path, text)
    with pytest.raises(ValueError, match=match):
        parse_genbank_file(p, length_check=False)
    if case in ("remote", "gap", "one_of"):
        return          # the reference reads such a key line as a continuation of the previous feature's last qualifier
    with pytest.raises(R.RStop):      # the reference stops on the others too
        R.parse_genbank(R.read_lines(open(p, "rb").read()))


def test_declared_divergence_mixed_strand_join(tmp_path):
    """join(complement(..), complement(..)) and join(a, complement(b)): the reference's regexes give an NA start (or drop segments) and
    GRanges fails on the file; the native parser gives each segment its own strand."""
    seq = _seq(100, 5)
    p = _write(tmp_path, _gbk([_feature("CDS", "join(complement(4..10),complement(1..3))"), _feature("CDS", "join(20..30,complement(40..50))")],
                              seq))
    assert _rows(_quiet(p)) == [(4, 10, "-"), (1, 3, "-"), (20, 30, "+"), (40, 50, "-")]
    with pytest.raises(R.RStop):
        R.parse_genbank(R.read_lines(open(p, "rb").read()))


def test_exports_and_estimate_arguments():
    import ldweaver_amd
    assert ldweaver_amd.parse_genbank_file is parse_genbank_file and "GenBankRecord" in ldweaver_amd.__all__
    with pytest.raises(NotImplementedError):
        cds.estimate_variation_in_CDS(None, gbk={"gbk": object(), "ref_g": 1})
    with pytest.raises(NotImplementedError):
        cds.estimate_variation_in_CDS(None, gbk={"ref_g": 1})


# ---------------------------------------------------------------------------------------------------------------------------------------
# random files against the literal port
# ---------------------------------------------------------------------------------------------------------------------------------------
def _rand_range(rng, g):
    a = int(rng.integers(1, g))
    kind = rng.integers(0, 6)
    if kind == 0:
        return str(a)
    if kind == 1:
        return f"{a}^{a + 1}"
    b = a - 2 if rng.random() < 0.004 else int(rng.integers(a - 1, min(g, a + 400) + 1))      # a - 2: negative width
    lt, gt = ("<" if rng.random() < 0.1 else ""), (">" if rng.random() < 0.1 else "")
    return f"{lt}{a}..{gt}{b}"


def _rand_location(rng, g):
    k = rng.integers(0, 6)
    if k <= 1:
        loc = _rand_range(rng, g)
    else:
        op = "join" if k <= 3 else "order"
        loc = f"{op}(" + ",".join(_rand_range(rng, g) for _ in range(int(rng.integers(1, 5)))) + ")"
    if rng.random() < 0.35:
        loc = f"complement({loc})"
    parts = loc.split(",")
    if len(parts) > 1 and rng.random() < 0.4:       # over several lines, broken after a comma
        return [x + "," for x in parts[:-1]] + [parts[-1]]
    return loc


def _rand_file(rng):
    g = int(rng.integers(200, 3000))
    seq = "".join(rng.choice(list("acgtACGTNn-" if rng.random() < 0.5 else "acgt"), size=g))
    tab = rng.random() < 0.2
    feats = []
    for j in range(int(rng.integers(0, 25))):
        key = rng.choice(["CDS", "CDS", "CDS", "gene", "misc_feature", "tRNA", "rRNA", "repeat_region"])
        quals = []
        if rng.random() < 0.8:
            quals.append(f'/locus_tag="R_{j:04d}"')
        if rng.random() < 0.5:
            quals.append(f'/gene="g{j}x"')
        if rng.random() < 0.6:
            quals.append(("/product=\"putative", "protein " + str(j) + "\"") if rng.random() < 0.5 else f'/product="protein {j}"')
        if key == "CDS" and rng.random() < 0.5:
            aa = "".join(rng.choice(list("ACDEFGHIKLMNPQRSTVWY"), size=int(rng.integers(5, 150))))
            quals.append(["/translation=\"" + aa[:44]] + [aa[i:i + 58] for i in range(44, len(aa), 58)])
            quals[-1][-1] += '"'
        if rng.random() < 0.2:
            quals.append("/pseudo")
        if rng.random() < 0.2:
            quals.append("/transl_table=11")
        feats.append(_feature(key, _rand_location(rng, g), quals, tab=tab))
    src_len = g if rng.random() < 0.7 else int(rng.integers(1, g + 1))
    tail = "BASE COUNT      10 a     20 c     30 g     40 t\n" if rng.random() < 0.3 else ""
    text = _gbk(feats, seq, source=f"1..{src_len}", tail=tail)
    eol = rng.choice(["\n", "\r\n", "\r"])
    name = "r.gbk.gz" if rng.random() < 0.25 else "r.gbk"
    return text, eol, name


def test_random_files_match_the_literal_port(tmp_path):
    rng = np.random.default_rng(2024)
    n_rows = n_err = 0
    for i in range(200):
        text, eol, name = _rand_file(rng)
        p = _write(tmp_path, text, name=f"{i}_{name}", eol=eol)
        try:
            lit = R.parse_genbank(R.read_lines(open(p, "rb").read()))
        except R.RStop as e:
            lit = e
        try:
            rec = _quiet(p)
        except ValueError as e:
            rec = e
        if isinstance(lit, Exception):
            assert isinstance(rec, Exception), (i, lit)
            n_err += 1
            continue
        assert not isinstance(rec, Exception), (i, rec)
        assert _rows(rec) == lit["rows"], i
        assert rec.cds["seqnames"].tolist() == lit["seqnames"]
        tags = [tuple("" if v is True else v for v in t) for t in lit["tags"]]
        assert list(rec.cds[["locus_tag", "gene", "product"]].itertuples(index=False, name=None)) == [tags[k] for k in lit["feature"]]
        assert rec.sequence.tobytes().decode() == lit["sequence"]
        n_rows += len(lit["rows"])
    assert n_rows > 1000 and 5 < n_err < 100          # both paths are exercised (negative widths are the errors here)


# ---------------------------------------------------------------------------------------------------------------------------------------
# a bacterial-scale file
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_parse_time_bacterial_scale(tmp_path):
    rng = np.random.default_rng(9)
    g = 5_000_000
    seq = rng.choice(np.frombuffer(b"acgt", dtype=np.uint8), size=g).tobytes().decode()
    feats = []
    starts = np.sort(rng.choice(np.arange(1, g - 3000), size=5000, replace=False))
    for j, s in enumerate(starts.tolist()):
        e = s + int(rng.integers(100, 2000))
        loc = f"complement({s}..{e})" if j % 2 else f"{s}..{e}"
        aa = "".join(rng.choice(list("ACDEFGHIKLMNPQRSTVWY"), size=(e - s) // 3))
        tr = ["/translation=\"" + aa[:44]] + [aa[i:i + 58] for i in range(44, len(aa), 58)]
        tr[-1] += '"'
        feats.append(_feature("gene", loc, [f'/locus_tag="B_{j:05d}"']))
        feats.append(_feature("CDS", loc, [f'/locus_tag="B_{j:05d}"', '/product="hypothetical protein"', "/codon_start=1", tr]))
    text = _gbk(feats, seq)
    times = {}
    for name in ("big.gbk", "big.gbk.gz"):
        p = _write(tmp_path, text, name=name)
        read_genbank(p)              # warm the page cache
        t0 = time.perf_counter()
        rec = read_genbank(p)
        times[name] = time.perf_counter() - t0
        assert len(rec.cds) == 5000 and rec.g == g and rec.cds["locus_tag"].iloc[-1] == "B_04999"
        assert rec.sequence[:10].tobytes() == seq[:10].upper().encode()
    print(f"\nparse of {len(text) / 1e6:.1f} MB GenBank (5 Mb, 5000 CDS): plain {times['big.gbk'] * 1e3:.0f} ms, "
          f"gzip {times['big.gbk.gz'] * 1e3:.0f} ms")
    assert max(times.values()) < 2.0
