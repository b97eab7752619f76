"""The parts of the pipeline driver that need no GPU (ldweaver_amd/driver.py): the argument checks and fall-backs of
``LDWeaver`` (R/BacGWES.R:99-192) and ``cleanup`` (R/io_functions.R:236-350) on a fabricated folder."""
import os
import warnings

import numpy as np
import pytest

from ldweaver_amd import driver as D

SNP = dict(aln_has_all_bases=False, pos=[3, 9, 27], gbk_path="a.gbk")


def _error(**kw):
    with pytest.raises(ValueError) as e:
        D.check_arguments(**kw)
    return str(e.value)


def test_check_arguments_errors():
    assert _error() == "Either gbk_path or gff3_path must be provided"
    assert _error(gbk_path="a.gbk", gff3_path="a.gff3", ref_fasta_path="a.fa") == "Either gbk_path or gff3_path must be provided"
    assert _error(gff3_path="a.gff3") == "Reference fasta file must be provided for gff3 annoations"
    assert _error(aln_has_all_bases=False, gbk_path="a.gbk") == "A numeric vector of 'positions' <pos> must be provided if aln_has_all_bases = F"
    assert _error(aln_has_all_bases=False, pos=["1", "2"], gbk_path="a.gbk") == "Provided pos must be numeric!"
    assert _error(aln_has_all_bases=False, pos=[1, 2, 2], gbk_path="a.gbk") == "Provided pos contains duplicates!"
    assert _error(pos=[1, 2], gbk_path="a.gbk").startswith("pos cannot be provided for alignments with all bases!")
    # LDWeaver itself raises them before anything else happens: no folder is made
    from ldweaver_amd import LDWeaver
    with pytest.raises(ValueError, match="Either gbk_path or gff3_path"):
        LDWeaver("no_such_dset_folder", "no_such.fa")
    assert not os.path.exists("no_such_dset_folder")


def test_check_arguments_defaults_pass_unchanged():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        a = D.check_arguments(gbk_path="a.gbk")
        b = D.check_arguments(gff3_path="a.gff3", ref_fasta_path="r.fa", SnpEff_Annotate=False, tanglegram_break_segments=None, **{k: SNP[k] for k in ("aln_has_all_bases", "pos")})
    assert a == dict(pos=None, order_links=False, sr_dist=20000, lr_retain_links=1e6, max_tophits=250, num_clusts_CDS=3, srp_cutoff=3,
                     tanglegram_break_segments=5, max_blk_sz=10000, validate_ref_ann_lengths=True)
    assert b["order_links"] is True and b["validate_ref_ann_lengths"] is False and b["tanglegram_break_segments"] is None
    assert np.array_equal(b["pos"], [3, 9, 27])


@pytest.mark.parametrize("name,bad,used", [
    ("sr_dist", 999, 1001), ("sr_dist", 100001, 99999), ("lr_retain_links", 1e3, 1e6), ("lr_retain_links", 1e10, 1e6),
    ("max_tophits", 49, 250), ("max_tophits", 1001, 250), ("num_clusts_CDS", 0, 3), ("num_clusts_CDS", 11, 3), ("srp_cutoff", -1, 3),
    ("srp_cutoff", 5.5, 3), ("tanglegram_break_segments", -1, 5), ("tanglegram_break_segments", 11, 5), ("max_blk_sz", 999, 10000),
    ("max_blk_sz", 100001, 10000)])
def test_check_arguments_warns_and_falls_back(name, bad, used):
    with pytest.warns(UserWarning, match=f"<{name}>"):
        a = D.check_arguments(gbk_path="a.gbk", **{name: bad})
    assert a[name] == used
    if name == "max_tophits":          # the reference assigns sr_dist = 250 here; we set max_tophits and leave sr_dist alone
        assert a["sr_dist"] == 20000
    # the limits themselves pass
    edge = {"sr_dist": (1000, 100000), "lr_retain_links": (1001, 1e6), "max_tophits": (50, 1000), "num_clusts_CDS": (1, 10), "srp_cutoff": (0, 5),
            "tanglegram_break_segments": (0, 10), "max_blk_sz": (1000, 100000)}[name]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for v in edge:
            assert D.check_arguments(gbk_path="a.gbk", **{name: v})[name] == v


def test_large_lr_retain_links_only_warns():
    with pytest.warns(UserWarning, match="very large lr_links.tsv"):
        assert D.check_arguments(gbk_path="a.gbk", lr_retain_links=2e6)["lr_retain_links"] == 2e6


# ---- cleanup -----------------------------------------------------------------------------------------------------------------------------------

ENTRIES = {
    "Fit": ["c1_fit_data.tsv", "c10_fit_data.tsv", "c2_fit_data.rds", "c1_fit.png", "c10_fit.png", "CDS_clustering.png"],
    "Additional_Outputs": ["snp_ACGTN.npz", "cds_var.npz", "hdw.npy"],
    "Annotated_links": ["sr_links_annotated.tsv", "lr_links_annotated.tsv"],
    "GWESPlots": ["sr_gwes_clust.png", "sr_gwes_combi.png", "lr_gwes.png"],
    "Tophits": ["sr_tophits.tsv", "lr_tophits.tsv", "SR_network_plot.png", "lr_network_plot.png"],
    "Temp": ["snpEff_out.txt", "sr_snps.vcf", "sr_annotations.tsv", "sr_links.tsv", "lr_links.tsv", "LDW_run_20240101000000.txt"],
}
DIRS = {"SR_GWESExplorer": {"snps.loci": "1\n2\n", "sub/deep.txt": "deep"}, "LR_GWESExplorer": {"snps.aln": ">a\nAC\n"}}
STAY = ["LD_plot.png", "SR_Tanglegram/tng_1.png", "notes_fit.png.bak", "c_fit.png"]


def _fabricate(root):
    root.mkdir()
    for names in ENTRIES.values():
        for n in names:
            (root / n).write_text("new " + n)
    for d, files in DIRS.items():
        for f, text in files.items():
            (root / d / f).parent.mkdir(parents=True, exist_ok=True)
            (root / d / f).write_text(text)
    for n in STAY:
        (root / n).parent.mkdir(parents=True, exist_ok=True)
        (root / n).write_text("stays " + n)
    (root / "Temp").mkdir()
    (root / "Temp" / "sr_links.tsv").write_text("from an earlier run")


def _tree(root):
    out = {}
    for base, _dirs, files in os.walk(root):
        for f in files:
            p = os.path.join(base, f)
            out[os.path.relpath(p, root)] = open(p).read()
    return out


@pytest.mark.parametrize("delete", [False, True])
def test_cleanup_sorts_the_folder(tmp_path, capsys, delete):
    root = tmp_path / "dset"
    _fabricate(root)
    moved = D.cleanup(str(root), delete_after_moving=delete)
    said = capsys.readouterr().out
    assert said.startswith("Cleaning up...\n")
    assert [ln for ln in said.splitlines() if ln.startswith("Not overwriting:")] == [f"Not overwriting: {root / 'sr_links.tsv'}"]
    want = {}
    for folder, names in ENTRIES.items():
        for n in names:
            want[f"{folder}/{n}"] = "new " + n
    want["Temp/sr_links.tsv"] = "from an earlier run"            # kept, not overwritten
    for d, files in DIRS.items():
        for f, text in files.items():
            want[f"GWESExplorer/{d}/{f}"] = text
    for n in STAY:
        want[n] = "stays " + n
    if not delete:
        for names in ENTRIES.values():
            for n in names:
                want[f"OLD/{n}"] = "new " + n                    # the new sr_links.tsv is still here
        for d, files in DIRS.items():
            for f, text in files.items():
                want[f"OLD/{d}/{f}"] = text
    assert _tree(root) == want
    top = set(os.listdir(root))
    assert top == {"Fit", "Additional_Outputs", "Annotated_links", "GWESPlots", "Tophits", "GWESExplorer", "Temp", "LD_plot.png", "SR_Tanglegram",
                   "notes_fit.png.bak", "c_fit.png"} | (set() if delete else {"OLD"})
    assert moved["c10_fit.png"] == str(root / "Fit" / "c10_fit.png") and moved["SR_GWESExplorer"] == str(root / "GWESExplorer" / "SR_GWESExplorer")
    assert "LD_plot.png" not in moved and "SR_Tanglegram" not in moved
    # a second call finds nothing to sort and changes nothing
    assert D.cleanup(str(root), delete_after_moving=delete) == {} and _tree(root) == want


def test_cleanup_overwrites_in_old_and_refuses_a_missing_folder(tmp_path, capsys):
    root = tmp_path / "dset"
    root.mkdir()
    (root / "OLD").mkdir()
    (root / "OLD" / "sr_tophits.tsv").write_text("older")
    (root / "sr_tophits.tsv").write_text("newer")
    D.cleanup(str(root))
    assert (root / "OLD" / "sr_tophits.tsv").read_text() == "newer" and (root / "Tophits" / "sr_tophits.tsv").read_text() == "newer"
    with pytest.raises(FileNotFoundError, match="not found!"):
        D.cleanup(str(tmp_path / "nothing_here"))


def test_cleanup_sweeps_the_two_snpeff_files_of_the_working_directory(tmp_path, monkeypatch, capsys):
    work = tmp_path / "work"
    work.mkdir()
    (work / "snpEff_genes.txt").write_text("genes")
    (work / "snpEff_summary.html").write_text("<html>")
    (work / "other.txt").write_text("other")
    root = tmp_path / "dset"
    root.mkdir()
    monkeypatch.chdir(work)
    D.cleanup(str(root))
    assert sorted(os.listdir(work)) == ["other.txt"]
    assert (root / "Temp" / "snpEff_genes.txt").read_text() == "genes" and (root / "Temp" / "snpEff_summary.html").read_text() == "<html>"


def test_saved_intermediates_round_trip(tmp_path):
    from ldweaver_amd.snpdat import CdsVar, SnpDat
    rng = np.random.default_rng(2)
    st = rng.integers(0, 5, (6, 4)).astype(np.uint8)
    sd = SnpDat.from_states(st, [5, 9, 11, 40, 41, 77], g=None, seq_names=["a", "b", "c", "d"])
    D.save_snp_dat(str(tmp_path / "snp_ACGTN.npz"), sd, st)
    back = D.load_snp_dat(str(tmp_path / "snp_ACGTN.npz"))
    assert back.g is None and np.array_equal(back.states, st) and np.array_equal(back.POS, sd.POS) and back.seq_names == sd.seq_names
    assert np.array_equal(back.uqe, sd.uqe) and np.array_equal(back.r, sd.r) and (back.nsnp, back.nseq) == (6, 4)
    sd.g = 100.0
    D.save_snp_dat(str(tmp_path / "snp_ACGTN.npz"), sd, st)
    assert D.load_snp_dat(str(tmp_path / "snp_ACGTN.npz")).g == 100.0
    cv = CdsVar(paint=np.array([1, 1, 2, 2, 3, 3]), nclust=3, var_estimate=np.array([0.1, 0.2]), cds_start=np.array([1, 30]), cds_end=np.array([20, 90]),
                clusts={"km_clst_ord": np.array([1, 2], dtype=np.int32), "cutoff": 0.1}, ref=np.array(list("ACGTac")), alt=["C", "A,G", "T", "*", "A", "C,T"],
                allele_table=rng.integers(0, 4, (5, 6)).astype(np.int32))
    D.save_cds_var(str(tmp_path / "cds_var.npz"), cv)
    b = D.load_cds_var(str(tmp_path / "cds_var.npz"))
    assert b.nclust == 3 and b.alt == cv.alt and np.array_equal(b.ref, cv.ref) and np.array_equal(b.paint, cv.paint)
    assert np.array_equal(b.clusts["km_clst_ord"], [1, 2]) and b.clusts["cutoff"] == 0.1 and np.array_equal(b.allele_table, cv.allele_table)
    # a SnpDat whose alignment stayed on the device still knows its shape
    assert (SnpDat(states=None, POS=sd.POS, g=None, uqe=sd.uqe, r=sd.r, seq_names=["a", "b"]).nsnp, SnpDat(states=None, POS=sd.POS, g=None, uqe=sd.uqe, r=sd.r,
                                                                                                          seq_names=["a", "b"]).nseq) == (6, 2)
