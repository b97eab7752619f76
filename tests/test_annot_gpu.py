"""GPU: perform_snpEff_annotations (ldweaver_amd/annotate.py, csrc/ldw_annot.hip) against the port of tests/annot_ref.py: hand-built GenBank
and GFF genomes that hit every effect on both strands, 200 random genomes, the golden sample through perform_MI_computation (SR and LR, both
routes, byte-identical files, tophits that feed the GWESExplorer writer), and 10^6 links against a vectorised numpy route by SHA-256."""
import hashlib
import os
import warnings

import numpy as np
import pandas as pd
import pytest

import annot_ref as ref
from ldweaver_amd import annotate as A
from ldweaver_amd import extract
from ldweaver_amd import lr as LR
from ldweaver_amd import mi as MIH
from ldweaver_amd import output as O
from ldweaver_amd import rcompat
from ldweaver_amd.cds import Annotation, estimate_variation_in_CDS
from ldweaver_amd.engine import Engine
from ldweaver_amd.gbk import parse_genbank_file
from ldweaver_amd.snpdat import CdsVar, SnpDat

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEAD = ("LOCUS       TST0001                 {g} bp    DNA     circular BCT 01-JAN-2024\n"
        "DEFINITION  Testus syntheticus.\nACCESSION   TST0001\nVERSION     TST0001.1\nKEYWORDS    .\nSOURCE      Testus syntheticus\n"
        "  ORGANISM  Testus syntheticus\n            Bacteria.\nFEATURES             Location/Qualifiers\n")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def gbk_text(seq: str, feats) -> str:
    """feats: (segments [(lo, hi)], strand, locus_tag or "", gene or "")"""
    out = [HEAD.format(g=len(seq)), f"     source          1..{len(seq)}\n", '                     /organism="Testus syntheticus"\n']
    for segs, strand, lt, gene in feats:
        loc = ",".join(f"{a}..{b}" for a, b in segs)
        loc = f"join({loc})" if len(segs) > 1 else loc
        loc = f"complement({loc})" if strand < 0 else loc
        out.append(f"     CDS             {loc}\n")
        if lt:
            out.append(f'                     /locus_tag="{lt}"\n')
        if gene:
            out.append(f'                     /gene="{gene}"\n')
    out.append("ORIGIN      \n")
    for i in range(0, len(seq), 60):
        c = seq[i:i + 60].lower()
        out.append(f"{i + 1:>9} " + " ".join(c[j:j + 10] for j in range(0, len(c), 10)) + "\n")
    return "".join(out) + "//\n"


def ref_feats(feats, seqname):
    out = []
    for i, (segs, strand, lt, gene) in enumerate(feats):
        lo, hi = min(a for a, _ in segs), max(b for _, b in segs)
        gid = lt or f"{seqname}:{lo}-{hi}"
        out.append(ref.feature(list(segs), strand, gid, gene or gid, i))
    return out


def dev_feats(feats):
    seg, strand = [], []
    for f, (segs, sd, _, _) in enumerate(feats):
        seg += [(a, b, f) for a, b in sorted(segs, reverse=sd < 0)]
        strand.append(sd)
    return np.array(seg, np.int32).reshape(-1, 3), np.array(strand, np.int8)


def _mask(alt):
    return sum(1 << "ACGT".index(a) for a in alt.split(",") if a in "ACGT")


# ---- the hand-built genome ----------------------------------------------------------------------------------------------------------------
# + gene A (1..15, ATG GCT TGG CAA TAA), - gene B on 31..45 (coding ATG GCT TGG CAA TAA), a join() gene C (61..66 + 70..78: ATG AAA TTT
# GGG TAA... ), overlapping D/E, an N inside F and F's incomplete last codon, far features for intergenic at both ends.
def hand_genome():
    rng = np.random.default_rng(5)
    g = 30000
    s = list(rng.choice(list("ACGT"), g))

    def put(at, text):
        s[at - 1:at - 1 + len(text)] = list(text)
    put(1, "ATGGCTTGGCAATAA")
    put(31, ref.revcomp("ATGGCTTGGCAATAA"))
    put(61, "ATGAAA" + "CCC" + "TTTGGGTAA")        # C: 61..66 + 70..78 -> ATG AAA TTT GGG TAA
    put(100, "GTGCAGCAGCAGTGA")                    # D 100..114, E 106..120 overlaps it (+1 frame: start at 106)
    put(200, "ATGNCCTAGGC")                        # F 200..210: an N in codon 2, 11 bases (incomplete last codon)
    put(20000, "ATGTTTTAA")                        # G far right (+)
    put(9000, ref.revcomp("ATGTTTTAA"))            # H - strand, 9000..9008
    feats = [([(1, 15)], 1, "tagA", "aaa"), ([(31, 45)], -1, "tagB", ""), ([(61, 66), (70, 78)], 1, "", "ccc"), ([(100, 114)], 1, "tagD", "ddd"),
             ([(106, 120)], 1, "tagE", ""), ([(200, 210)], 1, "tagF", "fff"), ([(20000, 20008)], 1, "tagG", "ggg"),
             ([(9000, 9008)], -1, "tagH", "hhh")]
    snps = {2: "C", 3: "A", 1: "G", 6: "A", 9: "A", 10: "C", 12: "A", 13: "C", 14: "G", 15: "A",   # A: start lost/retained, syn, stop...
            44: "C", 43: "A", 33: "C", 32: "T", 36: "C", 42: "A",                              # B on the complement
            64: "C", 71: "G", 74: "A", 67: "T",                                                 # C across the join, 67 in its gap
            108: "T", 110: "C", 203: "A", 204: "G", 209: "C", 210: "T",                          # D/E overlap, F's N and incomplete codon
            20: "A", 50: "G", 2000: "T", 8000: "C", 9010: "A", 8990: "A", 14000: "G", 14500: "A", 19990: "C", 20020: "A", 29990: "T",
            300: "*", 5: "*", 400: "A,*", 7: "A,G,T"}
    seq = "".join(s)
    seq = seq[:299] + seq[299].lower() + seq[300:]     # a lower-case base
    return seq, feats, snps


def test_hand_genome_every_effect(eng, tmp_path):
    seq, feats, snps = hand_genome()
    pos = np.array(sorted(snps), np.int32)
    alts = [snps[p] for p in pos.tolist()]
    for src in ("gbk", "gff"):
        if src == "gbk":
            p = tmp_path / "h.gbk"
            p.write_text(gbk_text(seq, feats))
            rec = parse_genbank_file(str(p), g=len(seq))["gbk"]
            f = A.features_of(gbk=rec)
            rseq = rec.sequence
            rf = ref_feats(feats, rec.seqname)
        else:
            rows = []
            for i, (segs, sd, lt, gene) in enumerate(feats):
                attrs = ";".join(x for x in (f"ID=f{i}", f"locus_tag={lt}" if lt else "", f"gene={gene}" if gene else "") if x)
                for a, b in segs:
                    rows.append(["chr1", ".", "CDS", a, b, ".", "+" if sd > 0 else "-", "0", attrs])
            df = pd.DataFrame(rows, columns=["seqid", "source", "type", "start", "end", "score", "strand", "phase", "attributes"])
            ann = Annotation(gff=df, ref=np.frombuffer(seq.encode(), np.uint8).copy(), ref_name="chr1", g=len(seq))
            f = A.features_of(gff=ann)
            rseq = ann.ref
            rf = [ref.feature(list(segs), sd, lt or f"f{i}", gene or lt or f"f{i}", i) for i, (segs, sd, lt, gene) in enumerate(feats)]
        seg, strand = dev_feats(feats)
        assert np.array_equal(f["seg"], seg) and np.array_equal(f["strand"], strand)
        rec_ = eng.annot_snps(rseq, f["seg"], f["strand"], pos, [_mask(a) for a in alts])
        got = A.native_table(rec_, f, pos)
        sref = bytes(rseq).decode()
        seen = set()
        for i, (p_, a) in enumerate(zip(pos.tolist(), alts)):
            an, n, gid, hc, hp = ref.native_annotation(sref, rf, p_, a)
            seen.add(an)
            assert (got["annotation"][i], got["description"][i], got["cds"][i]) == (an, ref.paste_unique([n, gid, hc, hp]), gid), (src, p_)
        assert seen >= {"start_lost", "start_retained_variant", "stop_gained", "stop_lost", "stop_retained_variant", "synonymous_variant",
                        "missense_variant", "coding_sequence_variant", "upstream_gene_variant", "downstream_gene_variant", "intergenic_region"}
    i = pos.tolist().index(300)
    assert got["description"][i].endswith(":") and got["annotation"][i] != "coding_sequence_variant"


def random_genome(rng):
    g = int(rng.integers(300, 4000))
    s = rng.choice(list("ACGTacgtN"), g, p=[0.22, 0.22, 0.22, 0.22, 0.025, 0.025, 0.025, 0.025, 0.02])
    seq = "".join(s)
    feats = []
    for i in range(int(rng.integers(0, 9))):
        nseg = int(rng.choice([1, 1, 1, 2, 3]))
        lo = int(rng.integers(1, g - 10))
        segs = []
        for _ in range(nseg):
            hi = min(g, lo + int(rng.integers(0, 400)))
            segs.append((lo, hi))
            lo = hi + int(rng.integers(1, 50))
            if lo >= g:
                break
        feats.append((segs, int(rng.choice([1, -1])), f"t{i}" if rng.random() < 0.7 else "", f"g{i}" if rng.random() < 0.5 else ""))
    pos = np.unique(rng.integers(1, g + 1, int(rng.integers(1, 60)))).astype(np.int32)
    alts = [",".join(sorted(set(rng.choice(list("ACGT*"), int(rng.integers(1, 4)))), key="ACGT*".index)) for _ in pos]
    return seq, feats, pos, alts


def test_random_genomes(eng):
    rng = np.random.default_rng(2024)
    for case in range(200):
        seq, feats, pos, alts = random_genome(rng)
        seg, strand = dev_feats(feats)
        rf = ref_feats(feats, "chr")
        f = dict(seg=seg, strand=strand, gene_id=[x["id"] for x in rf], gene_name=[x["name"] for x in rf])
        rec = eng.annot_snps(np.frombuffer(seq.encode(), np.uint8), seg, strand, pos, [_mask(a) for a in alts])
        got = A.native_table(rec, f, pos)
        for i, (p_, a) in enumerate(zip(pos.tolist(), alts)):
            an, n, gid, hc, hp = ref.native_annotation(seq, rf, p_, a)
            assert (got["annotation"][i], got["description"][i], got["cds"][i]) == (an, ref.paste_unique([n, gid, hc, hp]), gid), (case, p_, a)


# ---- the golden sample through perform_MI_computation --------------------------------------------------------------------------------------

def _expected_files(snp_dat, cv, links, genome, feats_ref, seq, links_type, max_tophits, ann_rows=None):
    POS = np.asarray(snp_dat.POS)
    snps = np.unique(np.concatenate([links["pos1"].to_numpy(float), links["pos2"].to_numpy(float)]))
    idx = [int(np.flatnonzero(POS == p)[0]) for p in snps]
    REF = [str(cv.ref[j]) for j in idx]
    ALT = [str(cv.alt[j]) for j in idx]
    vcf = ref.vcf_file(genome, snp_dat.g, snps, REF, ALT)
    if ann_rows is None:
        ann_rows = ref.native_ann_rows(seq, feats_ref, snps, REF, ALT, cv.allele_table, idx, snp_dat.nseq)
    d = {c: links[c].tolist() for c in ("pos1", "pos2", "len", "ARACNE", "MI") + (("srp_max",) if links_type == "SR" else ())}
    rows = ref.add_annotations_to_links(d, ann_rows, links_type)
    top = ref.detect_top_hits(rows, max_tophits)
    return dict(vcf=vcf, ann=ref.ann_tsv(ann_rows), links=ref.links_tsv(rows, links_type), top=ref.links_tsv(top, links_type)), ann_rows, vcf


def _files(folder, t):
    return dict(vcf=open(os.path.join(folder, f"{t}_snps.vcf")).read(), ann=open(os.path.join(folder, f"{t}_annotations.tsv")).read(),
                links=open(os.path.join(folder, f"{t}_links_annotated.tsv")).read(), top=open(os.path.join(folder, f"{t}_tophits.tsv")).read())


def _ann_vcf(vcf_text, seq, feats):
    """an annotated VCF as snpEff shapes it (16 fields per entry), carrying the port's native annotation (for the VCF route)"""
    out = []
    for line in vcf_text.splitlines(True):
        if line.startswith("#"):
            out.append(line)
            continue
        f = line.rstrip("\n").split("\t")
        an, n, gid, hc, hp = ref.native_annotation(seq, feats, int(f[1]), f[4])
        f[7] = f"ANN={f[4]}|{an}|MODIFIER|{n}|{gid}|transcript|{gid}|protein_coding|1/1|{hc}|{hp}|1/9|1/9|1/3||"
        out.append("\t".join(f) + "\n")
    return "".join(out)


def _snp_idx(sd, ann_rows):
    POS = np.asarray(sd.POS)
    return [int(np.flatnonzero(POS == int(r["pos"]))[0]) for r in ann_rows]


@pytest.fixture(scope="module")
def golden_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("golden")
    pos = np.loadtxt(os.path.join(GOLDEN, "snp_sample.pos"), dtype=np.int64)
    rng = np.random.default_rng(91)
    g = 50000
    seq = "".join(rng.choice(list("ACGT"), g))
    feats, at, i = [], 1, 0
    while at < g - 1500:                      # CDSs tiled over the genome, both strands, every fourth a join()
        ln = int(rng.integers(100, 400)) * 3
        if i % 4 == 3:
            segs = [(at, at + ln // 2 - 1), (at + ln // 2 + 30, at + ln + 29)]
        else:
            segs = [(at, at + ln - 1)]
        feats.append((segs, 1 if i % 3 else -1, f"LT_{i:04d}", f"gen{i}" if i % 2 else ""))
        at = segs[-1][1] + int(rng.integers(20, 900))
        i += 1
    p = tmp / "g.gbk"
    p.write_text(gbk_text(seq, feats))
    rec = parse_genbank_file(str(p), g=g)["gbk"]
    eng = Engine(0)
    sd = extract.parse_fasta_SNP_alignment(os.path.join(GOLDEN, "snp_sample.fa.gz"), pos, engine=eng)
    sd.g = float(g)
    cv = estimate_variation_in_CDS(sd, gbk=rec, engine=eng, alignment_resident=True)
    hdw = MIH.estimate_Hamming_distance_weights(sd, engine=eng, alignment_resident=True, verbose=False)
    red = MIH.perform_MI_computation(sd, hdw, cv, lr_save_path=str(tmp / "lr.tsv"), sr_save_path=str(tmp / "sr.tsv"), plt_folder=str(tmp / "P"),
                                     engine=eng, alignment_resident=True, verbose=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lr = LR.analyse_long_range_links(eng, sd, red, cv)["lr_links_red"]
    yield dict(eng=eng, sd=sd, cv=cv, red=red, lr=lr, rec=rec, seq=seq, feats=ref_feats(feats, rec.seqname), tmp=tmp)
    eng.close()


@pytest.mark.parametrize("links_type", ["SR", "LR"])
def test_golden_sample_both_routes(golden_run, links_type, tmp_path):
    G = golden_run
    links = G["red"] if links_type == "SR" else G["lr"]
    assert len(links) > 20
    t = links_type.lower()
    top = A.perform_snpEff_annotations("dset", str(tmp_path / "n"), "snpEff.jar", G["sd"], G["cv"], links, gbk={"gbk": G["rec"]},
                                       max_tophits=40, links_type=links_type, engine=G["eng"])
    want, ann_rows, vcf = _expected_files(G["sd"], G["cv"], links, "TST0001.1", G["feats"], G["seq"], links_type, 40)
    got = _files(tmp_path / "n", t)
    for k in want:
        assert got[k] == want[k], k
    assert 0 < len(top) <= 40 and list(top.columns) == want["top"].splitlines()[0].split("\t")
    assert set(top["links"]) <= set(A.PAIRS) and "syXsy" not in set(top["links"])
    # the VCF route on a snpEff-shaped file of the same annotations gives the same table, links and tophits
    (tmp_path / "v").mkdir()
    annotated = _ann_vcf(vcf, G["seq"], G["feats"])
    (tmp_path / "v" / f"{t}_snps_ann.vcf").write_text(annotated)
    A.perform_snpEff_annotations("dset", str(tmp_path / "v"), "snpEff.jar", G["sd"], G["cv"], links, gbk=G["rec"], max_tophits=40,
                                 links_type=links_type, engine=G["eng"], annotator="vcf")
    gv = _files(tmp_path / "v", t)
    want_v, _, _ = _expected_files(G["sd"], G["cv"], links, "TST0001.1", None, None, links_type, 40,
                                   ann_rows=ref.convert_vcfann_to_table(annotated, _snp_idx(G["sd"], ann_rows), G["cv"].allele_table, G["sd"].nseq))
    for k in want_v:
        assert gv[k] == want_v[k], k
    assert gv["links"] == got["links"] and gv["top"] == got["top"]
    # the tophits feed the GWESExplorer writer unchanged
    O.write_output_for_gwes_explorer(G["sd"], top, str(tmp_path / "gw"), links_type=links_type, engine=G["eng"], alignment_resident=True)
    th = O.read_TopHits(str(tmp_path / "n" / f"{t}_tophits.tsv"))
    O.write_output_for_gwes_explorer(G["sd"], th, str(tmp_path / "gw2"), links_type=links_type, engine=G["eng"], alignment_resident=True)
    for f in ("snps.loci", "snps.aln", "snps.outliers"):
        assert (tmp_path / "gw" / f).read_bytes() == (tmp_path / "gw2" / f).read_bytes(), f


def test_single_snp_and_gff_route(eng, tmp_path):
    """one annotated SNP (R's ncol() of a dropped vector fails there: a declared divergence), GFF input"""
    seq = "ATGGCTTGGCAATAA" + "A" * 85
    ann = Annotation.from_arrays([1], [15], seq, ref_name="c9")
    sd = SnpDat(states=np.zeros((3, 4), np.uint8), POS=np.array([5, 40, 60], np.int32), g=100.0, uqe=np.ones((3, 5)), r=np.full(3, 2))
    cv = CdsVar(paint=np.ones(3, np.int32), nclust=1, ref=np.array(["C", "A", "A"]), alt=["T", "C", "G"],
                allele_table=np.array([[0, 3, 3], [3, 1, 0], [0, 0, 1], [1, 0, 0], [0, 0, 0]], np.int32))
    links = pd.DataFrame({"pos1": [5.0, 5.0], "pos2": [5.0, 5.0], "len": [0.0, 0.0], "MI": [0.2, 0.3], "ARACNE": [1, 1]})
    top = A.perform_snpEff_annotations("d", str(tmp_path), "j", sd, cv, links, gff=ann, links_type="LR", engine=eng)
    assert len(top) == 0      # both ends in one gene region
    got = _files(tmp_path, "lr")
    # (ALT is one "T": type.convert makes the column logical, as read.table of the VCF would)
    assert got["ann"] == "pos\tREF\tALT\tannotation\tdescription\tcds\tcode\tallele_dist\n" \
                         "5\tC\tTRUE\tmissense_variant\tc9:1-15:c.5C>T:p.Ala2Val\tc9:1-15\tns\tC:0.75, T:0.25\n"
    assert got["links"].splitlines()[1] == "5\t5\t0\tTRUE\t0.3\tc9:1-15:c.5C>T:p.Ala2Val\tc9:1-15:c.5C>T:p.Ala2Val\tc9:1-15\tc9:1-15\tnsXns\t" \
                                           "C:0.75, T:0.25\tC:0.75, T:0.25"


# ---- ldw_annot_map with the positions in any order ------------------------------------------------------------------------------------------------

def test_annot_map_with_positions_in_any_order(eng):
    POS = np.array([40, 10, 30, 70, 50, 20], dtype=np.int32)
    pos1, pos2 = np.array([10.0, 70.0, 10.0]), np.array([40.0, 20.0, 70.0])
    ends = np.unique(np.r_[pos1, pos2])                                     # the annotation rows: the distinct link positions, ascending
    order = np.argsort(POS, kind="stable")
    want = order[np.searchsorted(POS[order], ends)]
    snp, bad = eng.annot_map(pos1, pos2, POS)
    assert len(ends) == 4 and snp.tolist() == want.tolist() == [1, 5, 0, 3] and bad == -1
    # a position two SNPs hold is nobody's: the first such end, e < n in pos1 and n + i in pos2
    TWICE = np.array([40, 10, 30, 10], dtype=np.int32)
    assert eng.annot_map([40.0, 30.0], [30.0, 10.0], TWICE)[1] == 2 + 1
    assert eng.annot_map([40.0, 10.0], [30.0, 10.0], TWICE)[1] == 1
    # a fractional end lies between two positions: compared as a double, never rounded onto a SNP
    assert eng.annot_map([10.5], [40.0], POS)[1] == 0
    assert eng.annot_map([40.0], [10.5], POS)[1] == 1
    # one SNP, linked to itself
    snp, bad = eng.annot_map([5.0], [5.0], np.array([5], dtype=np.int32))
    assert snp.tolist() == [0] and bad == -1


# ---- 10^6 links ---------------------------------------------------------------------------------------------------------------------------

def test_million_links_sha256(eng, tmp_path):
    rng = np.random.default_rng(11)
    g, nsnp, n = 200000, 5000, 1_000_000
    seq = "".join(rng.choice(list("ACGT"), g))
    POS = np.sort(rng.choice(np.arange(1, g + 1), nsnp, replace=False)).astype(np.int32)
    feats, at, i = [], 1, 0
    while at < g - 2000:
        ln = int(rng.integers(100, 500)) * 3
        feats.append(([(at, at + ln - 1)], 1 if i % 2 else -1, f"LT{i}", ""))
        at += ln + int(rng.integers(0, 3000))
        i += 1
    ann = Annotation.from_arrays([f[0][0][0] for f in feats], [f[0][0][1] for f in feats], seq)
    ann.gff["strand"] = ["+" if f[1] > 0 else "-" for f in feats]
    ann.gff["attributes"] = [f"locus_tag={f[2]}" for f in feats]
    refc = np.array([seq[p - 1] for p in POS])
    alts = [str(rng.choice([a for a in "ACGT" if a != r])) for r in refc]
    at_ = rng.integers(0, 50, (5, nsnp)).astype(np.int32)
    sd = SnpDat(states=np.zeros((nsnp, 50), np.uint8), POS=POS, g=float(g), uqe=np.ones((nsnp, 5)), r=np.full(nsnp, 2))
    cv = CdsVar(paint=np.ones(nsnp, np.int32), nclust=1, ref=refc, alt=alts, allele_table=at_)
    a = rng.integers(0, nsnp, n)
    b = rng.integers(0, nsnp, n)
    srp = np.round(rng.random(n) * 50, 1)
    srp[rng.random(n) < 0.001] = np.nan
    links = pd.DataFrame({"pos1": POS[a].astype(float), "pos2": POS[b].astype(float), "len": np.abs(POS[a] - POS[b]).astype(float),
                          "MI": np.round(rng.random(n), 6), "srp_max": srp, "ARACNE": (rng.random(n) < 0.7).astype(float)})
    top = A.perform_snpEff_annotations("d", str(tmp_path), "j", sd, cv, links, gff=ann, max_tophits=500, engine=eng)
    # the numpy route: the per-SNP table from the device's own annotations file, the join / order / filter vectorised
    at = pd.read_csv(tmp_path / "sr_annotations.tsv", sep="\t", quoting=3, keep_default_na=False, dtype=str)
    apos = at["pos"].to_numpy(np.int64)
    r1 = np.searchsorted(apos, links["pos1"].to_numpy(np.int64))
    r2 = np.searchsorted(apos, links["pos2"].to_numpy(np.int64))
    order = np.argsort(-links["srp_max"].to_numpy(), kind="stable")
    desc, cds, code, ad = (at[c].to_numpy(object) for c in ("description", "cds", "code", "allele_dist"))

    def fmt(col):
        u, inv = np.unique(col, return_inverse=True)
        return np.array([rcompat.format_number(x) for x in u], dtype=object)[inv]
    cols = [links["pos1"].to_numpy(np.int64).astype(str).astype(object), links["pos2"].to_numpy(np.int64).astype(str).astype(object),
            fmt(links["len"].to_numpy()), fmt(links["ARACNE"].to_numpy()), fmt(links["MI"].to_numpy()), fmt(links["srp_max"].to_numpy()),
            desc[r1], desc[r2], cds[r1], cds[r2], code[r1] + "X" + code[r2], ad[r1], ad[r2]]
    cols = [c[order] for c in cols]
    body = cols[0]
    for c in cols[1:]:
        body = body + "\t" + c
    text = "\t".join(A.SR_COLS) + "\n" + "\n".join(body.tolist()) + "\n"
    assert hashlib.sha256(text.encode()).hexdigest() == hashlib.sha256((tmp_path / "sr_links_annotated.tsv").read_bytes()).hexdigest()
    keep = (links["ARACNE"].to_numpy()[order] == 1) & (cols[10] != "syXsy") & (cols[8] != cols[9]) & (cols[8] != "NA") & (cols[9] != "NA")
    sel = np.flatnonzero(keep)[:500]
    top_text = "\t".join(A.SR_COLS) + "\n" + "".join(x + "\n" for x in body[sel].tolist())
    assert (tmp_path / "sr_tophits.tsv").read_text() == top_text
    assert len(top) == len(sel) == 500
