"""GPU: estimate_variation_in_CDS from a GenBank file (ldweaver_amd.gbk) — the same CDSs and reference written as GenBank and as GFF3 plus
FASTA give bit-identical cds_var, equal to the literal port of tests/cds_ref.py; a lower-case ORIGIN still masks the reference allele; and the
pipeline FASTA -> GenBank -> cds_var -> perform_MI_computation on one resident engine against the oracle."""
import os
import warnings

import numpy as np
import pandas as pd
import pytest

import cds_ref as R
import ldw_oracle as orc
from ldweaver_amd import _lib as L
from ldweaver_amd import extract
from ldweaver_amd import mi as MIH
from ldweaver_amd.cds import estimate_variation_in_CDS, parse_gff_file
from ldweaver_amd.gbk import parse_genbank_file
from ldweaver_amd.snpdat import SnpDat
from test_cds_gpu import _compare_literal, _golden_cds, _kmeans_cluster, _write_fasta
from test_gbk_host import _feature, _gbk

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MI_TIGHT = 1e-10


def _annotation_files(tmp_path, POS, g, rng, ref: bytes, lower_origin=False):
    """The CDS list of _golden_cds(special=False) plus a complement(join(...)) CDS and an a^b site, written as GenBank and as GFF3 rows in
    the same order; returns (gbk path, gff path, fasta path, starts, ends)."""
    st, en = _golden_cds(POS, g, rng, special=False)
    keep = en >= st
    st, en = st[keep], en[keep]
    sp = np.sort(POS)
    feats, rows = [], []
    for j, (s, e) in enumerate(zip(st.tolist(), en.tolist())):
        loc = f"complement({s}..{e})" if j % 4 == 1 else (f"{s}..{e}" if j % 3 else f"<{s}..>{e}")
        feats.append(_feature("CDS", loc, [f'/locus_tag="T_{j:03d}"', '/product="hypothetical protein"']))
        rows.append((s, e))
        if j == 3:
            a, b, c, d = int(sp[50]) - 20, int(sp[60]) + 3, int(sp[80]) - 7, int(sp[90]) + 11
            feats.append(_feature("CDS", [f"complement(join({a}..{b},", f"{c}..{d}))"], ['/locus_tag="T_join"']))
            rows += [(a, b), (c, d)]
            x = int(sp[120])
            feats.append(_feature("CDS", f"{x}^{x + 1}", ['/locus_tag="T_site"']))
            rows.append((x, x))
    seq = ref.decode()
    gbk = tmp_path / "a.gbk"
    gbk.write_text(_gbk(feats, seq.lower() if lower_origin else seq))
    lines = ["##gff-version 3"] + [f"ref1\ttest\tCDS\t{s}\t{e}\t.\t+\t0\tID=cds{j}" for j, (s, e) in enumerate(rows)]
    (tmp_path / "a.gff3").write_text("\n".join(lines) + "\n")
    _write_fasta(tmp_path / "ref.fa", b"ref1", ref)
    starts, ends = (np.array(v, dtype=np.int64) for v in zip(*rows))
    return str(gbk), str(tmp_path / "a.gff3"), str(tmp_path / "ref.fa"), starts, ends


def _upper_reference(g, rng):
    alpha = np.frombuffer(b"ACGTN-RY", dtype=np.uint8)
    p = np.array([0.23] * 4 + [0.03, 0.03, 0.01, 0.01])
    return alpha[rng.choice(len(alpha), size=g, p=p / p.sum())].tobytes()


def _same(a, b):
    assert np.array_equal(a.var_estimate, b.var_estimate) and np.array_equal(a.cds_start, b.cds_start) and np.array_equal(a.cds_end, b.cds_end)
    assert np.array_equal(a.clusts["km_clst_ord"], b.clusts["km_clst_ord"]) and a.clusts["cutoff"] == b.clusts["cutoff"]
    assert a.ref.tolist() == b.ref.tolist() and a.alt == b.alt and np.array_equal(a.paint, b.paint)
    assert np.array_equal(a.allele_table, b.allele_table)


def test_genbank_equals_gff_and_literal(engine, sample, tmp_path):
    rng = np.random.default_rng(43)
    st, POS, g = sample["states"], sample["POS"], 50000
    ref = _upper_reference(g, rng)
    gbk_p, gff_p, fa_p, starts, ends = _annotation_files(tmp_path, POS, g, rng, ref)
    parsed = parse_genbank_file(gbk_p, g=g)
    rec = parsed["gbk"]
    assert parsed["ref_g"] == g and rec.sequence.tobytes() == ref
    assert np.array_equal(rec.cds["start"].to_numpy(), starts) and np.array_equal(rec.cds["end"].to_numpy(), ends)
    assert (rec.cds["strand"] == "-").sum() >= 3 and "T_join" in rec.cds["locus_tag"].tolist()
    ann = parse_gff_file(gff_p, fa_p)
    sd = SnpDat.from_states(st, POS, float(g))
    engine.set_alignment(st)
    counts = orc.acgtn_table(st)
    for quirk in (L.QUIRK_REFERENCE, L.QUIRK_INTENDED):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # (a last SNP alone in its run warns the same on both routes; the paint is compared)
            cv_g = estimate_variation_in_CDS(sd, gbk=parsed, engine=engine, alignment_resident=True, quirk_mode=quirk)
            cv_r = estimate_variation_in_CDS(sd, gbk=rec, engine=engine, alignment_resident=True, quirk_mode=quirk)
            cv_f = estimate_variation_in_CDS(sd, gff=ann, engine=engine, alignment_resident=True, quirk_mode=quirk)
        _same(cv_g, cv_f)
        _same(cv_g, cv_r)
        lit = R.estimate_literal(list(POS), counts, ref, list(starts), list(ends), 3, _kmeans_cluster, quirk)
        _compare_literal(cv_g, lit)
        assert len(cv_g.var_estimate) >= 20


def test_lower_case_origin_masks_the_reference(engine, sample, tmp_path):
    rng = np.random.default_rng(44)
    st, POS, g = sample["states"], sample["POS"], 50000
    ref = _upper_reference(g, rng)
    gbk_p, _, _, starts, ends = _annotation_files(tmp_path, POS, g, rng, ref, lower_origin=True)
    parsed = parse_genbank_file(gbk_p, g=g)
    assert parsed["gbk"].sequence.tobytes() == ref
    engine.set_alignment(st)
    sd = SnpDat.from_states(st, POS, float(g))
    cv = estimate_variation_in_CDS(sd, gbk=parsed, engine=engine, alignment_resident=True)
    refs = cv.ref.tolist()
    assert all(c.isupper() or c in "-" for c in refs) and sum(c in "ACGT" for c in refs) > 0.8 * len(refs)
    for r, a in zip(refs, cv.alt):
        if r in "ACGT":
            assert r not in a.split(","), (r, a)
    lit = R.estimate_literal(list(POS), orc.acgtn_table(st), ref, list(starts), list(ends), 3, _kmeans_cluster)
    _compare_literal(cv, lit)


def test_pipeline_fasta_genbank_cds_var_mi(engine, tmp_path):
    pos = np.loadtxt(os.path.join(GOLDEN, "snp_sample.pos"), dtype=np.int64)
    sd = extract.parse_fasta_SNP_alignment(os.path.join(GOLDEN, "snp_sample.fa.gz"), pos, engine=engine)
    assert sd.g is None
    rng = np.random.default_rng(78)
    g = 50000
    ref = _upper_reference(g, rng)
    gbk_p, _, _, _, _ = _annotation_files(tmp_path, sd.POS, g, rng, ref)
    with pytest.warns(UserWarning, match="NOT checked"):
        parsed = parse_genbank_file(gbk_p, g=sd.g, length_check=False)
    sd.g = float(parsed["ref_g"])                  # R/BacGWES.R:338-342
    cv = estimate_variation_in_CDS(sd, gbk=parsed, engine=engine, alignment_resident=True)
    assert cv.nclust == 3 and set(cv.paint.tolist()) == {1, 2, 3}
    hdw = MIH.estimate_Hamming_distance_weights(sd, engine=engine, alignment_resident=True, verbose=False)
    lr_p, sr_p = str(tmp_path / "lr.tsv"), str(tmp_path / "sr.tsv")
    red = MIH.perform_MI_computation(sd, hdw, cv, ncores=1, lr_save_path=lr_p, sr_save_path=sr_p, plt_folder=str(tmp_path / "plots"),
                                     engine=engine, alignment_resident=True, verbose=False)
    st = sd.states
    ref_out = orc.perform_mi_computation(st, sd.POS, sd.g, sd.r, sd.uqe, hdw, cv.paint, 3, lr_retain_links=1e6, max_blk_sz=10000)
    rr = ref_out.sr_links_red
    assert len(red) == len(rr["MI"]) > 100
    ko = np.lexsort((np.asarray(rr["clust_c"]), rr["pos2"], rr["pos1"]))
    kg = np.lexsort((red["clust_c"].to_numpy(), red["pos2"].to_numpy(), red["pos1"].to_numpy()))
    for k in ("clust_c", "pos1", "pos2", "clust1", "clust2", "len"):
        assert np.array_equal(red[k].to_numpy(dtype=float)[kg], np.asarray(rr[k], dtype=float)[ko]), k
    assert np.abs(red["MI"].to_numpy()[kg] - rr["MI"][ko]).max() < MI_TIGHT
    assert np.abs(red["srp_max"].to_numpy()[kg] - rr["srp_max"][ko]).max() < 1e-6
    lr_lines = open(lr_p).read().splitlines()
    assert len(lr_lines) == len(ref_out.lr_rows["MI"])
    first = lr_lines[0].split("\t")
    assert float(first[0]) == ref_out.lr_rows["pos1"][0] and abs(float(first[5]) - ref_out.lr_rows["MI"][0]) < 1e-9
    lr_tab = pd.read_csv(lr_p, sep="\t", header=None)
    assert np.array_equal(lr_tab[2].to_numpy(dtype=float), np.asarray(ref_out.lr_rows["clust1"], dtype=float))
    assert np.array_equal(lr_tab[3].to_numpy(dtype=float), np.asarray(ref_out.lr_rows["clust2"], dtype=float))
    srl = open(sr_p).read().splitlines()
    assert len(srl) == len(red) and len(srl[0].split("\t")) == 9
