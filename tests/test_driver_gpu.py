"""The pipeline driver end to end (ldweaver_amd/driver.py) on the bundled SNP sample with a synthetic 50 kb GenBank file — the
inputs of test_annot_gpu.py's golden run: ``LDWeaver()`` must leave exactly what the same public step functions leave when they are called by
hand in its order, sort the folder as ``cleanup`` says, and take the reference's resume branches on a second run.  Needs an MI355X."""
import os
import re
import warnings

import numpy as np
import pytest

import plot_ref as R
from test_annot_gpu import gbk_text

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
pytestmark = pytest.mark.gpu
FOLDERS = {"Fit", "Additional_Outputs", "Annotated_links", "GWESPlots", "Tophits", "GWESExplorer", "Temp"}


def _genbank(path):
    """The 50 kb record of test_annot_gpu.py::golden_run (same seed): CDSs tiled over both strands, every fourth a join()."""
    rng = np.random.default_rng(91)
    g = 50000
    seq = "".join(rng.choice(list("ACGT"), g))
    feats, at, i = [], 1, 0
    while at < g - 1500:
        ln = int(rng.integers(100, 400)) * 3
        segs = [(at, at + ln // 2 - 1), (at + ln // 2 + 30, at + ln + 29)] if i % 4 == 3 else [(at, at + ln - 1)]
        feats.append((segs, 1 if i % 3 else -1, f"LT_{i:04d}", f"gen{i}" if i % 2 else ""))
        at = segs[-1][1] + int(rng.integers(20, 900))
        i += 1
    path.write_text(gbk_text(seq, feats))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """One driver run into <tmp>/drv and the chain by hand into <tmp>/hand, each on an engine of its own."""
    from ldweaver_amd import LDWeaver
    from ldweaver_amd import lr as LR
    from ldweaver_amd.annotate import perform_snpEff_annotations
    from ldweaver_amd.cds import estimate_variation_in_CDS
    from ldweaver_amd.driver import SMALL_LDMAP_REDUCER
    from ldweaver_amd.engine import Engine
    from ldweaver_amd.extract import parse_fasta_SNP_alignment
    from ldweaver_amd.gbk import parse_genbank_file
    from ldweaver_amd.mi import estimate_Hamming_distance_weights, perform_MI_computation
    from ldweaver_amd.network import create_network
    from ldweaver_amd.output import write_output_for_gwes_explorer
    from ldweaver_amd.plots import make_gwes_plots
    from ldweaver_amd.tanglegram import create_tanglegram
    tmp = tmp_path_factory.mktemp("driver")
    aln = os.path.join(GOLDEN, "snp_sample.fa.gz")
    pos = np.loadtxt(os.path.join(GOLDEN, "snp_sample.pos"), dtype=np.int64)
    gbk_path = tmp / "g.gbk"
    _genbank(gbk_path)
    dset = str(tmp / "drv")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = LDWeaver(dset, aln, aln_has_all_bases=False, pos=pos, gbk_path=str(gbk_path), save_additional_outputs=True, verbose=False)
        hand = str(tmp / "hand")
        os.makedirs(hand)
        h = lambda *p: os.path.join(hand, *p)      # noqa: E731
        with Engine(0) as eng:
            sd = parse_fasta_SNP_alignment(aln, pos, method="default", gap_freq=0.15, maf_freq=0.01, engine=eng, keep_on_device=True)
            gbk = parse_genbank_file(str(gbk_path), g=None, length_check=False)
            sd.g = float(gbk["ref_g"])
            cv = estimate_variation_in_CDS(sd, gbk=gbk, num_clusts_CDS=3, clust_plt_path=h("CDS_clustering.png"), engine=eng, alignment_resident=True)
            hdw = estimate_Hamming_distance_weights(sd, threshold=0.1, engine=eng, alignment_resident=True, verbose=False)
            sr = perform_MI_computation(sd, hdw, cv, lr_save_path=h("lr_links.tsv"), sr_save_path=h("sr_links.tsv"), plt_folder=hand, sr_dist=20000,
                                        lr_retain_links=1e6, max_blk_sz=10000, srp_cutoff=3, runARACNE=True, perform_SR_analysis_only=False,
                                        order_links=False, engine=eng, alignment_resident=True, verbose=False, fit_plots=True)
            # (the sample's links hold 1268 positions: the default reducer would be 1, the dense map, which the library does not draw; the driver uses 2)
            LR.genomewide_LDMap(eng, sd, reducer=SMALL_LDMAP_REDUCER, plot_save_path=h("LD_plot.png"), plot_title=f"GW-LD: {dset}",
                                lr_links_path=h("lr_links.tsv"), sr_links_path=h("sr_links.tsv"), sr_dist=20000)
            make_gwes_plots(lr_links=None, sr_links=sr, plt_folder=hand, are_srlinks_ordered=False, engine=eng)
            top = perform_snpEff_annotations(dset, hand, "snpEff.jar", sd, cv, sr, gbk=gbk, gbk_path=str(gbk_path), tophits_path=h("sr_tophits.tsv"),
                                             max_tophits=250, engine=eng, annotator="native")
            os.makedirs(h("SR_Tanglegram"))
            create_tanglegram(top, gbk=gbk, tanglegram_folder=h("SR_Tanglegram"), break_segments=5, engine=eng)
            os.makedirs(h("SR_GWESExplorer"))
            write_output_for_gwes_explorer(sd, top, h("SR_GWESExplorer"), engine=eng, alignment_resident=True)
            create_network(top, netplot_path=h("SR_network_plot.png"), plot_title=f"Networks in short-range tophits for {dset}", engine=eng)
            lr = LR.analyse_long_range_links(eng, sd, cds_var=cv, lr_plt_path=h("lr_gwes.png"), lr_links_path=h("lr_links.tsv"),
                                             sr_links_path=h("sr_links.tsv"), sr_dist=20000)["lr_links_red"]
            lr_top = perform_snpEff_annotations(dset, hand, "snpEff.jar", sd, cv, lr, gbk=gbk, gbk_path=str(gbk_path), tophits_path=h("lr_tophits.tsv"),
                                                max_tophits=500, links_type="LR", engine=eng, annotator="native")
            os.makedirs(h("LR_GWESExplorer"))
            write_output_for_gwes_explorer(sd, lr_top, h("LR_GWESExplorer"), links_type="LR", engine=eng, alignment_resident=True)
            create_network(lr_top, netplot_path=h("lr_network_plot.png"), plot_title=f"Networks in long-range tophits for {dset}", engine=eng)
    return dict(dset=dset, hand=hand, res=res, sr=sr, top=top, lr_top=lr_top, aln=aln, pos=pos, gbk_path=str(gbk_path), nclust=3)


def _bytes(*p):
    with open(os.path.join(*p), "rb") as fh:
        return fh.read()


def test_driver_equals_the_chain_by_hand(runs):
    d, h = runs["dset"], runs["hand"]
    assert len(runs["sr"]) > 20 and len(runs["top"]) > 0 and len(runs["lr_top"]) > 0
    pairs = [("Temp/sr_links.tsv", "sr_links.tsv"), ("Temp/lr_links.tsv", "lr_links.tsv"), ("Tophits/sr_tophits.tsv", "sr_tophits.tsv"),
             ("Tophits/lr_tophits.tsv", "lr_tophits.tsv"), ("Annotated_links/sr_links_annotated.tsv", "sr_links_annotated.tsv"),
             ("Annotated_links/lr_links_annotated.tsv", "lr_links_annotated.tsv"), ("Fit/CDS_clustering.png", "CDS_clustering.png"),
             ("GWESPlots/sr_gwes_clust.png", "sr_gwes_clust.png"), ("GWESPlots/sr_gwes_combi.png", "sr_gwes_combi.png"),
             ("GWESPlots/lr_gwes.png", "lr_gwes.png"), ("LD_plot.png", "LD_plot.png"), ("Tophits/SR_network_plot.png", "SR_network_plot.png"),
             ("Tophits/lr_network_plot.png", "lr_network_plot.png")]
    fits = sorted(f for f in os.listdir(h) if re.fullmatch(r"c[0-9]+_fit(_data\.tsv|\.png)", f))
    assert fits == [f"c{i}_fit{e}" for i in range(1, runs["nclust"] + 1) for e in (".png", "_data.tsv")]
    pairs += [(f"Fit/{f}", f) for f in fits]
    pairs += [(f"GWESExplorer/{k}_GWESExplorer/{f}", f"{k}_GWESExplorer/{f}") for k in ("SR", "LR") for f in ("snps.loci", "snps.aln", "snps.outliers")]
    tng = sorted(os.listdir(os.path.join(h, "SR_Tanglegram")))
    assert tng and sorted(os.listdir(os.path.join(d, "SR_Tanglegram"))) == tng
    pairs += [(f"SR_Tanglegram/{f}", f"SR_Tanglegram/{f}") for f in tng]
    for a, b in pairs:
        assert _bytes(d, a) == _bytes(h, b), (a, b)
    # the two new figures are figures
    for f in ("Fit/c1_fit.png", "Fit/CDS_clustering.png"):
        img, _ = R.png_decode(_bytes(d, f))
        assert img.shape == (1200, 2200, 3) and len({tuple(p) for p in img[::7, ::7].reshape(-1, 3)}) > 3


def test_the_folder_after_cleanup(runs):
    d, res = runs["dset"], runs["res"]
    assert set(os.listdir(d)) == FOLDERS | {"OLD", "LD_plot.png", "SR_Tanglegram"}
    assert sorted(os.listdir(os.path.join(d, "Additional_Outputs"))) == ["cds_var.npz", "hdw.npy", "snp_ACGTN.npz"]
    assert sorted(os.listdir(os.path.join(d, "GWESPlots"))) == ["lr_gwes.png", "sr_gwes_clust.png", "sr_gwes_combi.png"]
    assert sorted(os.listdir(os.path.join(d, "GWESExplorer"))) == ["LR_GWESExplorer", "SR_GWESExplorer"]
    temp = sorted(os.listdir(os.path.join(d, "Temp")))
    logs = [f for f in temp if f.startswith("LDW_run_")]
    assert len(logs) == 1 and set(temp) - set(logs) == {"lr_annotations.tsv", "lr_links.tsv", "lr_snps.vcf", "sr_annotations.tsv", "sr_links.tsv", "sr_snps.vcf"}
    # what the driver returns: every file where it now lies, and the seconds
    assert res["dset"] == os.path.abspath(d) and res["log"] == os.path.join(d, "Temp", logs[0])
    assert all(os.path.exists(p) for p in res["files"].values()), [p for p in res["files"].values() if not os.path.exists(p)]
    assert res["files"]["sr_tophits.tsv"] == os.path.join(d, "Tophits", "sr_tophits.tsv") and res["files"]["LD_plot.png"] == os.path.join(d, "LD_plot.png")
    assert res["files"]["c1_fit.png"] == os.path.join(d, "Fit", "c1_fit.png") and res["files"]["SR_GWESExplorer"] == os.path.join(d, "GWESExplorer", "SR_GWESExplorer")
    assert {f"block_{k}" for k in range(1, 13)} | {"total"} == set(res["timings"]) and all(v >= 0 for v in res["timings"].values())
    assert res["timings"]["total"] >= max(v for k, v in res["timings"].items() if k != "total")
    # the log: banners of the twelve blocks in order, the branch messages of a first run, and the closing line (written before cleanup moved the file)
    log = open(res["log"]).read()
    assert re.findall(r"#### BLOCK (\d+) ####", log) == [str(k) for k in range(1, 13)]
    for line in ("Parsing Alignment:", "Reading the GBK file, validate_length_check =  False", "Extracted ref genome length 50000 from genbank...",
                 "Estimating the variation in CDS", "Estimating per sequence Hamming distance", "Commencing MI computation", "** All done in"):
        assert line in log, line
    assert "Loading previous" not in log and "Cleaning up" not in log


def test_a_second_run_takes_the_resume_branches(runs):
    """The saved intermediates, the link files in Temp/ and the two tophits files are found where cleanup put them: nothing is recomputed, the
    figures that are drawn again are the same bytes, and the folder ends as it was."""
    from ldweaver_amd import LDWeaver
    d = runs["dset"]
    keep = {f: _bytes(d, f) for f in ("Temp/sr_links.tsv", "Temp/lr_links.tsv", "Tophits/sr_tophits.tsv", "Tophits/lr_tophits.tsv", "LD_plot.png",
                                      "GWESPlots/sr_gwes_clust.png", "GWESPlots/sr_gwes_combi.png", "Tophits/SR_network_plot.png")}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = LDWeaver(d, runs["aln"], aln_has_all_bases=False, pos=runs["pos"], gbk_path=runs["gbk_path"], save_additional_outputs=True, verbose=False)
    log = open(res["log"]).read()
    for line in ("Loading previous snp matrix", "Loading previous CDS variation estimates", "Loading previous Hamming distance estimates",
                 "Loading previous MI computation", "Loading previous top hits", "Results from previous LR anlayis exist!", "** All done in"):
        assert line in log, line
    assert "Commencing MI computation" not in log and "Parsing Alignment" not in log
    for f, b in keep.items():
        assert _bytes(d, f) == b, f
    assert set(os.listdir(d)) == FOLDERS | {"OLD", "LD_plot.png", "SR_Tanglegram"}
    assert len([f for f in os.listdir(os.path.join(d, "Temp")) if f.startswith("LDW_run_")]) in (1, 2)      # (2 unless both runs fell into one second)


def test_without_annotations_the_run_ends_at_block_8(runs, tmp_path):
    from ldweaver_amd import LDWeaver
    d = str(tmp_path / "plain")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = LDWeaver(d, runs["aln"], aln_has_all_bases=False, pos=runs["pos"], gbk_path=runs["gbk_path"], SnpEff_Annotate=False, verbose=False)
    assert set(os.listdir(d)) == {"Fit", "GWESPlots", "Temp", "OLD", "LD_plot.png"}
    assert sorted(os.listdir(os.path.join(d, "GWESPlots"))) == ["sr_gwes_clust.png", "sr_gwes_combi.png"]
    assert re.findall(r"#### BLOCK (\d+) ####", open(res["log"]).read()) == [str(k) for k in range(1, 9)]
    # order_links = True: the links are written in descending srp_max
    srp = np.loadtxt(os.path.join(d, "Temp", "sr_links.tsv"), usecols=7)
    assert len(srp) == len(runs["sr"]) and np.all(np.diff(srp) <= 0)
    assert _bytes(d, "LD_plot.png") != b"" and R.png_decode(_bytes(d, "LD_plot.png"))[0].shape == (5250, 5000, 3)


def test_an_empty_short_range_frame_stops_the_run(runs, tmp_path):
    """A run whose sr_links.tsv from an earlier run is empty takes the 'Loading previous' branch and stops after block 6, the log closed."""
    from ldweaver_amd import LDWeaver
    d = tmp_path / "empty"
    (d / "Temp").mkdir(parents=True)
    (d / "Temp" / "sr_links.tsv").write_text("")
    (d / "Temp" / "lr_links.tsv").write_bytes(_bytes(runs["dset"], "Temp/lr_links.tsv"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(RuntimeError) as e:
            LDWeaver(str(d), runs["aln"], aln_has_all_bases=False, pos=runs["pos"], gbk_path=runs["gbk_path"], verbose=False)
    assert str(e.value) == "No potentially important sr_links were identified! Cannot continue analysis..."
    logs = [f for f in os.listdir(d) if f.startswith("LDW_run_")]
    assert len(logs) == 1 and "BLOCK 6" in (d / logs[0]).read_text() and "BLOCK 7" not in (d / logs[0]).read_text()


# ---- a tiny full alignment with a GFF3 annotation ---------------------------------------------------------------------------------------------------------

TINY_SEED = 10     # the first seed for which the chain keeps a short-range link (seeds 0-9 end in the model's "no short-range link exceeds the fitted decay")


def tiny_job(folder, seed):
    """40 sequences x 3000 columns with 150 planted variable sites — most of them copies of six bipartitions of the sequences, so that sites in
    linkage lie within the short-range distance of each other —, eight CDSs in a GFF3 file, and the reference FASTA.  Returns the three paths."""
    rng = np.random.default_rng(seed)
    length, n = 3000, 40
    ref = rng.choice(list("ACGT"), length)
    aln = np.tile(ref, (n, 1))
    sites = np.sort(rng.choice(np.arange(20, length - 20), 150, replace=False))
    pats = rng.random((6, n)) < 0.4
    for j, s in enumerate(sites):
        p = pats[j % 6].copy() if rng.random() < 0.7 else rng.random(n) < 0.3
        p ^= rng.random(n) < 0.03
        if not p.any() or p.all():
            p[0] = not p[0]
        aln[p, s] = "ACGT"[("ACGT".index(ref[s]) + 1 + int(rng.integers(0, 3))) % 4]
    os.makedirs(folder, exist_ok=True)
    aln_path, ref_path, gff_path = (os.path.join(folder, f) for f in ("tiny.fa", "tiny_ref.fa", "tiny.gff3"))
    with open(aln_path, "w") as fh:
        for k in range(n):
            fh.write(f">iso_{k}\n{''.join(aln[k])}\n")
    with open(ref_path, "w") as fh:
        fh.write(">tiny\n" + "".join(ref) + "\n")
    with open(gff_path, "w") as fh:
        fh.write("##gff-version 3\n##sequence-region tiny 1 3000\n")
        for i in range(8):
            a = 31 + i * 360
            fh.write(f"tiny\tsynth\tCDS\t{a}\t{a + 299}\t.\t{'+' if i % 2 else '-'}\t0\tID=cds{i};Name=gene{i};locus_tag=T_{i:03d}\n")
    return aln_path, ref_path, gff_path


def test_full_alignment_with_gff3_short_range_only(tmp_path):
    from ldweaver_amd import LDWeaver
    aln, ref, gff = tiny_job(str(tmp_path / "in"), TINY_SEED)
    d = str(tmp_path / "tiny")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = LDWeaver(d, aln, gff3_path=gff, ref_fasta_path=ref, perform_SR_analysis_only=True, sr_dist=1000, srp_cutoff=0, verbose=False)
    assert set(os.listdir(d)) == {"Fit", "Annotated_links", "GWESPlots", "Tophits", "GWESExplorer", "Temp", "OLD", "SR_Tanglegram"}      # no LD map, no lr_*
    log = open(res["log"]).read()
    assert re.findall(r"#### BLOCK (\d+) ####", log) == ["1", "2", "3", "4", "5", "7", "8", "9", "10", "11"]
    assert "Only short-range analysis requested." in log and "Genomewide LD map cannot be plotted with only the short_range analysis." in log
    assert "Reading the gff3 file" in log and "Extracted ref genome length" not in log
    sr = np.loadtxt(os.path.join(d, "Temp", "sr_links.tsv"), ndmin=2)
    assert len(sr) >= 1 and sr.shape[1] == 9 and (sr[:, 5] < 1000).all() and (sr[:, 7] > 0).all()
    assert not os.path.exists(os.path.join(d, "Temp", "lr_links.tsv"))
    assert sorted(os.listdir(os.path.join(d, "Tophits"))) == ["SR_network_plot.png", "sr_tophits.tsv"]
    assert R.png_decode(_bytes(d, "Fit", "CDS_clustering.png"))[0].shape == (1200, 2200, 3)
    assert set(res["timings"]) == {f"block_{k}" for k in (1, 2, 3, 4, 5, 7, 8, 9, 10, 11)} | {"total"}
