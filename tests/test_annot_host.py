"""CPU tests of the SnpEff step (ldweaver_amd/annotate.py): the VCF bytes, convert_vcfann_to_table on hand-made snpEff ANN strings, the
allele distribution, R's text rules, the port's native rule table pinned by hand, every argument error before an engine exists, and the
string-table column kind of the native writer."""
import os

import numpy as np
import pandas as pd
import pytest

import annot_ref as ref
from ldweaver_amd import _lib as L
from ldweaver_amd import annotate as A
from ldweaver_amd.cds import Annotation
from ldweaver_amd.snpdat import CdsVar, SnpDat


def test_vcf_bytes_pinned():
    txt = A.vcf_text("NC_1.1", 2000000, np.array([5, 100000, 1234567]), ["A", "t", "G"], ["C", "A,*", "*"])
    want = ("##fileformat=VCF4.1\n##contig=<ID=1,length=2000000>\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
            "NC_1.1\t5\t.\tA\tC\t.\t.\t.\nNC_1.1\t100000\t.\tt\tA,*\t.\t.\t.\nNC_1.1\t1234567\t.\tG\t*\t.\t.\t.\n")
    assert txt == want
    assert txt == ref.vcf_file("NC_1.1", 2000000, [5, 100000, 1234567], ["A", "t", "G"], ["C", "A,*", "*"])


ANN_VCF = """##fileformat=VCF4.1
##INFO=<ID=ANN,Number=.,Type=String,Description="Functional annotations">
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO
c1\t10\t.\tT\tC\t.\t.\tANN=C|missense_variant|MODERATE|dnaA|b0001|transcript|b0001|protein_coding|1/1|c.10T>C|p.Ser4Pro|10/900|10/900|4/299||,C|upstream_gene_variant|MODIFIER|dnaN|b0002|transcript|b0002|protein_coding||c.-50T>C|||||50|
c1\t20\t.\tT\tG\t.\t.\tANN="G|synonymous_variant|LOW|dnaA|b0001|transcript|b0001|protein_coding|1/1|c.20T>G|p.Leu7Leu|20/900|20/900|7/299||"
c1\t30\t.\tT\tA\t.\t.\tANN=A|downstream_gene_variant|MODIFIER|yaaA|yaaA|transcript|b0005|protein_coding||c.*40T>A|||||40|
c1\t40\t.\tT\tA,G\t.\t.\tANN=A|intergenic_region|MODIFIER|dnaA-dnaN|b0001-b0002|intergenic_region|b0001-b0002|||n.40T>A||||||
c1\t50\t.\tT\t*\t.\t.\t.
c1\t60\t.\tT\tA\t.\t.\tANN=A|stop_retained_variant&upstream_gene_variant|LOW|x|x|||||
c1\t70\t.\tT\tC\t.\t.\tANN=C|missense_variant|MODERATE|abc||transcript|t1|protein_coding|1/1|c.1T>C|p.Met1?
"""


def test_vcfann_table_hand_made(tmp_path):
    p = tmp_path / "ann.vcf"
    p.write_text(ANN_VCF)
    tab = A.vcfann_table(str(p))
    assert tab["pos"] == ["10", "20", "30", "40", "50", "60", "70"]
    assert tab["REF"] == ["TRUE"] * 7                      # an all-T REF column is logical TRUE after type.convert
    assert tab["ALT"] == ["C", "G", "A", "A,G", "*", "A", "C"]
    assert tab["annotation"] == ["missense_variant", "synonymous_variant", "downstream_gene_variant", "intergenic_region", None,
                                 "stop_retained_variant&upstream_gene_variant", "missense_variant"]
    assert tab["description"] == ["dnaA:b0001:c.10T>C:p.Ser4Pro", "dnaA:b0001:c.20T>G:p.Leu7Leu", "yaaA:c.*40T>A:",
                                  "dnaA-dnaN:b0001-b0002:n.40T>A:", "NA", "x:NA", "abc::c.1T>C:p.Met1?"]
    assert tab["cds"] == ["b0001", "b0001", "yaaA", "b0001-b0002", None, "x", ""]
    assert tab["code"] == ["ns", "sy", "ig", "ns", "ns", "ig", "ns"]
    at = np.array([[0, 1, 2, 3, 0, 5, 1], [5, 4, 3, 2, 0, 0, 1], [0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 5, 0, 1], [0, 0, 0, 0, 0, 0, 1]])
    want = ref.convert_vcfann_to_table(ANN_VCF, list(range(7)), at, 5)
    for k in ("pos", "REF", "ALT", "annotation", "description", "cds", "code"):
        assert tab[k] == [r[k] for r in want], k
    tab["allele_dist"] = A.allele_dist(at, np.arange(7), 5)
    assert tab["allele_dist"][:2] == ["C:1", "C:0.8, A:0.2"]
    assert tab["allele_dist"][6] == "A:0.2, C:0.2, G:0.2, T:0.2, N:0.2"      # equal counts keep A C G T N order
    assert A.annotations_text(tab) == ref.ann_tsv(want)
    assert A.annotations_text(tab).splitlines()[5] == "50\tTRUE\t*\tNA\tNA\tNA\tns\tT:1"


def test_r_text_rules():
    assert A.r_strsplit("a|b||") == ["a", "b", ""]
    assert A.r_strsplit("|a") == ["", "a"]
    assert A.r_strsplit("") == []
    assert A.r_paste_unique(["g", "g", "", ""]) == "g:"
    assert A.r_paste_unique([None, "x", None]) == "NA:x"
    assert A.type_convert(["1", "NA", "3"]) == ["1", None, "3"]
    assert A.type_convert(["T", "F"]) == ["TRUE", "FALSE"]
    assert A.type_convert(["1.5", "100000"]) == ["1.5", "1e+05"]
    assert A.type_convert(["A", "T"]) == ["A", "T"]
    assert [A.code_of(x) for x in ("synonymous_variant", "missense_variant&synonymous_variant", "upstream_gene_variant&synonymous_variant",
                                   "intergenic_region", "start_retained_variant", None)] == ["sy", "sy", "ig", "ns", "ns", "ns"]


def test_port_native_rules_pinned():
    # + strand CDS 1..12: ATG GCT TGG TAA; - strand CDS 31..39 on the complement
    seq = "ATGGCTTGGTAA" + "C" * 18 + "TTACCACAT" + "G" * 20
    f1 = ref.feature([(1, 12)], 1, "g1", "geneA", 0)
    f2 = ref.feature([(31, 39)], -1, "g2", "g2", 1)
    feats = [f1, f2]
    assert ref.native_annotation(seq, feats, 5, "T") == ("missense_variant", "geneA", "g1", "c.5C>T", "p.Ala2Val")
    assert ref.native_annotation(seq, feats, 6, "A") == ("synonymous_variant", "geneA", "g1", "c.6T>A", "p.Ala2Ala")
    assert ref.native_annotation(seq, feats, 9, "A") == ("stop_gained", "geneA", "g1", "c.9G>A", "p.Trp3*")
    assert ref.native_annotation(seq, feats, 11, "G") == ("stop_retained_variant", "geneA", "g1", "c.11A>G", "p.*4*")
    assert ref.native_annotation(seq, feats, 10, "C") == ("stop_lost", "geneA", "g1", "c.10T>C", "p.*4Glnext*?")
    assert ref.native_annotation(seq, feats, 1, "G") == ("start_retained_variant", "geneA", "g1", "c.1A>G", "p.Met1Met")
    assert ref.native_annotation(seq, feats, 2, "C") == ("start_lost", "geneA", "g1", "c.2T>C", "p.Met1?")
    # - strand: coding ATG TGG TAA read from 39 down; position 37 is c.3, 36 is c.4
    assert ref.native_annotation(seq, feats, 37, "A") == ("start_retained_variant", "g2", "g2", "c.3G>T", "p.Met1Met")
    assert ref.native_annotation(seq, feats, 36, "T") == ("missense_variant", "g2", "g2", "c.4T>A", "p.Trp2Arg")
    # non-coding: 20 is 8 after f1's end (downstream on +) and 11 before f2 (downstream on -: p < start)
    assert ref.native_annotation(seq, feats, 20, "A") == ("downstream_gene_variant", "geneA", "g1", "c.*8C>A", "")
    assert ref.native_annotation(seq, feats, 45, "A") == ("upstream_gene_variant", "g2", "g2", "c.-6C>T", "")
    assert ref.native_annotation(seq, feats, 10, "*") == ("coding_sequence_variant", "geneA", "g1", "", "")
    far = "A" * 30000
    g = [ref.feature([(6000, 6011)], 1, "L", "L", 0), ref.feature([(19000, 19011)], 1, "R", "R", 1)]
    assert ref.native_annotation(far, g, 12600, "C") == ("intergenic_region", "L-R", "L-R", "n.12600A>C", "")
    assert ref.native_annotation(far, g, 100, "C") == ("intergenic_region", "CHR_START-L", "CHR_START-L", "n.100A>C", "")
    assert ref.native_annotation(far, g, 29000, "G") == ("intergenic_region", "R-CHR_END", "R-CHR_END", "n.29000A>G", "")
    assert ref.native_annotation(far, g, 10000, "C") == ("downstream_gene_variant", "L", "L", "c.*3989A>C", "")


def test_native_features_gff(tmp_path):
    df = pd.DataFrame({"seqid": ["chr"] * 4, "source": ["."] * 4, "type": ["CDS", "cds", "gene", "CDS"], "start": [1, 20, 1, 40],
                       "end": [9, 30, 50, 48], "score": ["."] * 4, "strand": ["+", "+", "+", "-"], "phase": ["0"] * 4,
                       "attributes": ["ID=c%3B1;Name=nm", "ID=c%3B1", "ID=gene1", "locus_tag=lt2;gene=abc"]})
    ann = Annotation(gff=df, ref=np.frombuffer(b"A" * 60, dtype=np.uint8).copy(), ref_name="chr", g=60)
    f = A.features_of(gff=ann)
    assert f["seg"].tolist() == [[1, 9, 0], [20, 30, 0], [48 - 8, 48, 1]]
    assert f["strand"].tolist() == [1, -1]
    assert f["gene_id"] == ["c;1", "lt2"] and f["gene_name"] == ["nm", "abc"]


def _inputs(n_snp=6):
    POS = np.array([10, 20, 30, 40, 50, 60][:n_snp], dtype=np.int32)
    snp = SnpDat(states=np.zeros((n_snp, 4), np.uint8), POS=POS, g=100.0, uqe=np.ones((n_snp, 5)), r=np.full(n_snp, 2))
    cv = CdsVar(paint=np.ones(n_snp, np.int32), nclust=1, ref=np.array(["A"] * n_snp), alt=["C"] * n_snp,
                allele_table=np.ones((5, n_snp), np.int32))
    links = pd.DataFrame({"pos1": [10.0, 20.0], "pos2": [30.0, 40.0], "len": [20.0, 20.0], "MI": [0.5, 0.4], "srp_max": [3.0, 2.0],
                          "ARACNE": [1.0, 0.0]})
    ann = Annotation.from_arrays([1], [30], "A" * 100)
    return snp, cv, links, ann


def test_argument_errors_before_engine(tmp_path, monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError("an engine was made")
    monkeypatch.setattr(A, "Engine", no_engine)
    snp, cv, links, ann = _inputs()
    call = lambda **kw: A.perform_snpEff_annotations(**{**dict(dset_name="d", annotation_folder=str(tmp_path), snpeff_jar="snpEff.jar",
                                                              snp_dat=snp, cds_var=cv, links_df=links, gff=ann), **kw})
    with pytest.raises(ValueError, match="either one of gbk or gff"):
        call(gff=None)
    with pytest.raises(ValueError, match="either one of gbk or gff"):
        call(gbk=object())
    with pytest.raises(ValueError, match="LR or SR"):
        call(links_type="XR")
    with pytest.raises(ValueError, match="annotator"):
        call(annotator="snpeff")
    with pytest.raises(ValueError, match="max_tophits"):
        call(max_tophits=-1)
    with pytest.raises(ValueError, match="srp_max"):
        call(links_df=links.drop(columns="srp_max"))
    with pytest.raises(ValueError, match="empty"):
        call(links_df=links.iloc[:0])
    bad = links.copy()
    bad.loc[1, "pos2"] = 41.0
    with pytest.raises(ValueError, match=r"pos2 = 41 matches no SNP"):
        call(links_df=bad)
    snp2, _, _, _ = _inputs()
    snp2.POS = np.array([10, 20, 30, 30, 50, 60], dtype=np.int32)
    with pytest.raises(ValueError, match=r"pos2 = 30 matches several SNPs"):
        call(snp_dat=snp2)
    with pytest.raises(ValueError, match="cds_var"):
        call(cds_var=CdsVar(paint=cv.paint, nclust=1))
    # the VCF route without an annotated VCF: the VCF is written, the command line is named, nothing is run and no engine is made
    with pytest.raises(FileNotFoundError) as ei:
        call(annotator="vcf")
    msg = str(ei.value)
    assert "sr_snps_ann.vcf" in msg and "java -Xmx16G -jar 'snpEff.jar'" in msg and "sr_snps.vcf" in msg
    assert (tmp_path / "sr_snps.vcf").read_text() == ref.vcf_file("ref", 100, [10, 20, 30, 40], ["A"] * 4, ["C"] * 4)
    assert not os.path.exists(tmp_path / "sr_annotations.tsv")


def test_write_table_str_kind(tmp_path):
    lib = L.lib()
    import ctypes as C
    strings = ["", "alpha", "NA", "b:c:", "TRUE", "FALSE"]
    blob = "".join(strings).encode()
    offs = np.zeros(len(strings) + 1, np.int64)
    offs[1:] = np.cumsum([len(s) for s in strings])
    a = np.array([1, 100000, -3], np.int64)
    s1 = np.array([0, 1, 2], np.int32)
    s2 = np.array([1, 0, 1], np.int32)
    d = np.array([0.5, 1e-20, np.nan])
    kinds = np.array([L.COL_INT64, L.COL_STR, L.COL_DOUBLE, L.COL_STR], np.int32)
    cols = (C.c_void_p * 4)(a.ctypes.data, s1.ctypes.data, d.ctypes.data, s2.ctypes.data)
    base = np.array([0, 1, 0, 4], np.int64)
    p = tmp_path / "t.tsv"
    nb = C.c_int64()
    L.check(lib.ldw_write_table_tsv_str(os.fsencode(str(p)), 0, 3, 4, L.ptr(kinds), cols, L.ptr(base), blob, L.ptr(offs), len(strings), 2,
                                        C.byref(nb)))
    want = "1\talpha\t0.5\tFALSE\n100000\tNA\t1e-20\tTRUE\n-3\tb:c:\tNA\tFALSE\n"
    assert p.read_text() == want and nb.value == len(want)
    s1[2] = 5   # base 1 + 5 is outside the table
    assert lib.ldw_write_table_tsv_str(os.fsencode(str(p)), 0, 3, 4, L.ptr(kinds), cols, L.ptr(base), blob, L.ptr(offs), len(strings), 2,
                                       C.byref(nb)) == L.LDW_ERR_ARG
    # the numeric writer keeps refusing the new kind
    assert lib.ldw_write_table_tsv(os.fsencode(str(p)), 0, 3, 4, L.ptr(kinds), cols, 1, C.byref(nb)) == L.LDW_ERR_ARG
