"""The pipeline driver ``LDWeaver()`` (R/BacGWES.R:69-492) and ``cleanup()`` (R/io_functions.R:236-350): DESIGN.md 25.

``LDWeaver`` runs the reference's twelve blocks on ONE Engine: the alignment goes to the device in block 1 and stays there, every later step is
the package's public function called with ``alignment_resident=True``.  ``check_arguments`` holds the reference's checks and fall-backs and needs
no GPU; ``cleanup`` is file handling alone."""
from __future__ import annotations

import contextlib
import io
import os
import re
import shutil
import sys
import time
import warnings

import numpy as np

SR_EMPTY = "No potentially important sr_links were identified! Cannot continue analysis..."
ADDITIONAL = ("snp_ACGTN.npz", "cds_var.npz", "hdw.npy")
SMALL_LDMAP_REDUCER = 2      # block 6 where round(positions / 1000) <= 1
# folder, test of a top-level entry's name (the reference's patterns read as what they were meant to say: DESIGN.md 25)
CLEANUP_TABLE = (
    ("Fit", lambda f: re.search(r"^c[0-9]+_fit_data\.(tsv|rds)$", f) is not None),
    ("Additional_Outputs", lambda f: any(a in f for a in ADDITIONAL)),
    ("Fit", lambda f: re.search(r"^c[0-9]+_fit\.png$", f) is not None or "CDS_clustering.png" in f),
    ("Annotated_links", lambda f: "_links_annotated.tsv" in f),
    ("GWESPlots", lambda f: re.search(r"_gwes.+png", f) is not None),
    ("Tophits", lambda f: "_tophits.tsv" in f or "_network_plot.png" in f),
    ("GWESExplorer", lambda f: "_GWESExplorer" in f),
    ("Temp", lambda f: "snpEff" in f or re.search(r".vcf", f) is not None or "annotations.tsv" in f or "_links.tsv" in f or "LDW_run_" in f),
)
CLEANUP_FOLDERS = ("Fit", "Additional_Outputs", "Annotated_links", "GWESPlots", "Tophits", "GWESExplorer", "Temp")


# ---- cleanup ---------------------------------------------------------------------------------------------------------------------------------

def _copy(src, dst, overwrite: bool) -> bool:
    """``src`` (file or directory, recursively) to ``dst``; False when ``dst`` exists and may not be replaced."""
    if os.path.lexists(dst):
        if not overwrite:
            return False
        if os.path.isdir(dst) and not os.path.islink(dst):
            shutil.rmtree(dst)
        else:
            os.remove(dst)
    if os.path.isdir(src):
        shutil.copytree(src, dst)
    else:
        shutil.copy2(src, dst)
    return True


def _cleanup_support(paths, folder):
    os.makedirs(folder, exist_ok=True)
    for p in paths:
        if not _copy(p, os.path.join(folder, os.path.basename(p)), overwrite=False):
            print("Not overwriting:", p)


def cleanup(dset, delete_after_moving: bool = False) -> dict:
    """Sort the top-level entries of ``dset`` into the sub-folders of ``CLEANUP_TABLE`` (copied without overwriting: what is already there stays
    and is named in a ``Not overwriting:`` line); every sorted entry is then copied into ``OLD/`` (replacing what is there) unless
    ``delete_after_moving``, and removed from the top level.  ``LD_plot.png`` and ``SR_Tanglegram/`` stay where they are.  Returns
    {entry name: where it now lies} for the sorted entries."""
    print("Cleaning up...")
    dset = os.path.abspath(dset)
    if not os.path.exists(dset):
        raise FileNotFoundError(f"Dataset: {dset} not found!")
    files = sorted(f for f in os.listdir(dset) if f not in CLEANUP_FOLDERS and f != "OLD")
    moved = {}
    for folder, test in CLEANUP_TABLE:
        hit = [f for f in files if test(f)]
        if hit:
            _cleanup_support([os.path.join(dset, f) for f in hit], os.path.join(dset, folder))
            for f in hit:
                moved.setdefault(f, os.path.join(dset, folder, f))
    if moved:
        if not delete_after_moving:
            os.makedirs(os.path.join(dset, "OLD"), exist_ok=True)
            for f in sorted(moved):
                _copy(os.path.join(dset, f), os.path.join(dset, "OLD", f), overwrite=True)
        for f in moved:
            p = os.path.join(dset, f)
            if os.path.isdir(p) and not os.path.islink(p):
                shutil.rmtree(p)
            else:
                os.remove(p)
    # snpEff leaves two files in the working directory (R/io_functions.R:321-328)
    here = os.getcwd()
    stray = [f for f in sorted(os.listdir(here)) if "snpEff_genes.txt" in f or "snpEff_summary.html" in f]
    if stray:
        _cleanup_support([os.path.join(here, f) for f in stray], os.path.join(dset, "Temp"))
        for f in stray:
            os.remove(os.path.join(here, f))
    return moved


# ---- the checks of R/BacGWES.R:99-192 -------------------------------------------------------------------------------------------------------------

def check_arguments(aln_has_all_bases=True, pos=None, gbk_path=None, gff3_path=None, ref_fasta_path=None, validate_ref_ann_lengths=True,
                    SnpEff_Annotate=True, sr_dist=20000, lr_retain_links=1e6, max_tophits=250, num_clusts_CDS=3, srp_cutoff=3,
                    tanglegram_break_segments=5, max_blk_sz=10000) -> dict:
    """The reference's sanity checks (ValueError with its messages) and parameter fall-backs (a warning each); returns the values the run uses.
    No GPU, no file is touched.  ``max_tophits`` out of range falls back to 250 — the reference assigns ``sr_dist = 250`` there by mistake."""
    if (gbk_path is None) == (gff3_path is None):
        raise ValueError("Either gbk_path or gff3_path must be provided")
    if gff3_path is not None and ref_fasta_path is None:
        raise ValueError("Reference fasta file must be provided for gff3 annoations")
    order_links = not SnpEff_Annotate      # annotated links are ordered at the end, after the annotations are added
    if not aln_has_all_bases:
        if pos is None:
            raise ValueError("A numeric vector of 'positions' <pos> must be provided if aln_has_all_bases = F")
        try:
            p = np.asarray(pos)
        except Exception:
            p = np.asarray(pos, dtype=object)
        if p.dtype.kind not in "iuf" or p.ndim != 1:
            raise ValueError("Provided pos must be numeric!")
        if len(np.unique(p)) != len(p):
            raise ValueError("Provided pos contains duplicates!")
        pos = p
    elif pos is not None:
        raise ValueError("pos cannot be provided for alignments with all bases! Depending on the use case, either set pos = NULL or aln_has_all_bases = T")
    if sr_dist < 1000 or sr_dist > 100000:
        tmp = max(1001, min(99999, sr_dist))
        warnings.warn(f"Unable to use the provided value for <sr_dist>: {sr_dist} , instead using {tmp}", stacklevel=2)
        sr_dist = tmp
    if lr_retain_links <= 1e3 or lr_retain_links >= 1e10:
        warnings.warn("Unable to use the provided value for <lr_retain_links>, using 1e+06", stacklevel=2)
        lr_retain_links = 1e6
    if lr_retain_links > 1e6:
        warnings.warn("The given lr_retain_links value may generate a very large lr_links.tsv file!", stacklevel=2)
    if max_tophits < 50 or max_tophits > 1000:
        warnings.warn("Unable to use the provided value for <max_tophits>, using 250", stacklevel=2)
        max_tophits = 250
    if num_clusts_CDS < 1 or num_clusts_CDS > 10:
        warnings.warn("Unable to use the provided value for <num_clusts_CDS>, using 3", stacklevel=2)
        num_clusts_CDS = 3
    if srp_cutoff < 0 or srp_cutoff > 5:
        warnings.warn("Unable to use the provided value for <srp_cutoff>, using 3", stacklevel=2)
        srp_cutoff = 3
    if tanglegram_break_segments is not None and (tanglegram_break_segments < 0 or tanglegram_break_segments > 10):
        warnings.warn("Unable to use the provided value for <tanglegram_break_segments>, using 5", stacklevel=2)
        tanglegram_break_segments = 5
    if max_blk_sz < 1000 or max_blk_sz > 100000:
        warnings.warn("Unable to use the provided value for <max_blk_sz>, using 10000 ...!If this value is causing the function to crash, consider "
                      "reducing!...", stacklevel=2)
        max_blk_sz = 10000
    if not aln_has_all_bases:      # reference and alignment lengths cannot agree for a SNP-only alignment
        validate_ref_ann_lengths = False
    return dict(pos=pos, order_links=order_links, sr_dist=sr_dist, lr_retain_links=lr_retain_links, max_tophits=max_tophits,
                num_clusts_CDS=num_clusts_CDS, srp_cutoff=srp_cutoff, tanglegram_break_segments=tanglegram_break_segments, max_blk_sz=max_blk_sz,
                validate_ref_ann_lengths=bool(validate_ref_ann_lengths))


# ---- the saved intermediates (save_additional_outputs) ------------------------------------------------------------------------------------------------

def save_snp_dat(path, sd, states) -> None:
    """``snp_ACGTN.npz``: states (L, N) uint8, POS int32, g (NaN: unknown), uqe (L, 5), r (L), seq_names."""
    np.savez_compressed(path, states=np.asarray(states, dtype=np.uint8), POS=np.asarray(sd.POS, dtype=np.int32),
                        g=np.float64(np.nan if sd.g is None else sd.g), uqe=np.asarray(sd.uqe), r=np.asarray(sd.r),
                        seq_names=np.asarray(list(sd.seq_names), dtype=str))


def load_snp_dat(path):
    from .snpdat import SnpDat
    with np.load(path, allow_pickle=False) as z:
        g = float(z["g"])
        return SnpDat(states=z["states"], POS=z["POS"], g=None if np.isnan(g) else g, uqe=z["uqe"], r=z["r"], seq_names=[str(s) for s in z["seq_names"]])


def save_cds_var(path, cv) -> None:
    """``cds_var.npz``: paint, nclust, var_estimate, cds_start, cds_end, km_clst_ord, cutoff, ref, alt, allele_table."""
    np.savez_compressed(path, paint=np.asarray(cv.paint), nclust=np.int64(cv.nclust), var_estimate=np.asarray(cv.var_estimate),
                        cds_start=np.asarray(cv.cds_start), cds_end=np.asarray(cv.cds_end), km_clst_ord=np.asarray(cv.clusts["km_clst_ord"]),
                        cutoff=np.float64(cv.clusts["cutoff"]), ref=np.asarray(cv.ref, dtype=str), alt=np.asarray(list(cv.alt), dtype=str),
                        allele_table=np.asarray(cv.allele_table))


def load_cds_var(path):
    from .snpdat import CdsVar
    with np.load(path, allow_pickle=False) as z:
        return CdsVar(paint=z["paint"], nclust=int(z["nclust"]), var_estimate=z["var_estimate"], cds_start=z["cds_start"], cds_end=z["cds_end"],
                      clusts={"km_clst_ord": z["km_clst_ord"], "cutoff": float(z["cutoff"])}, ref=z["ref"], alt=[str(a) for a in z["alt"]],
                      allele_table=z["allele_table"])


# ---- the driver -------------------------------------------------------------------------------------------------------------------------------------------

class _Tee(io.TextIOBase):
    """What is printed during the run: into the log file and, unless quiet, on to the stream that was there."""

    def __init__(self, fh, out):
        self.fh, self.out = fh, out

    def write(self, s):
        self.fh.write(s)
        if self.out is not None:
            self.out.write(s)
        return len(s)

    def flush(self):
        self.fh.flush()
        if self.out is not None:
            self.out.flush()


def _first(*paths):
    """The last of ``paths`` that exists, else the first (a file may lie in ``dset`` or where an earlier cleanup put it)."""
    for p in paths[:0:-1]:
        if os.path.exists(p):
            return p
    return paths[0]


def LDWeaver(dset, aln_path, aln_has_all_bases=True, pos=None, gbk_path=None, gff3_path=None, ref_fasta_path=None, validate_ref_ann_lengths=True,
             snp_filt_method="default", gap_freq=0.15, maf_freq=0.01, hdw_threshold=0.1, perform_SR_analysis_only=False, SnpEff_Annotate=True,
             sr_dist=20000, lr_retain_links=1e6, max_tophits=250, num_clusts_CDS=3, srp_cutoff=3, tanglegram_break_segments=5, write_gwesExplorer=True,
             multicore=True, max_blk_sz=10000, ncores=None, save_additional_outputs=False, mega_dset=False, *, engine=None, annotator="native",
             verbose=True) -> dict:
    """The reference's ``LDWeaver()``: every output goes to the folder ``dset``, sorted by ``cleanup`` at the end.  ``multicore``, ``ncores`` and
    ``mega_dset`` are accepted and ignored.  ``engine``: the Engine to run on (one is made and closed otherwise); ``annotator``: as in
    ``perform_snpEff_annotations``; ``verbose=False`` prints nothing (the log file is written all the same).  Returns {"dset", "log", "files":
    {name: final path of every entry the run left in ``dset``}, "timings": seconds per block and in total}."""
    a = check_arguments(aln_has_all_bases, pos, gbk_path, gff3_path, ref_fasta_path, validate_ref_ann_lengths, SnpEff_Annotate, sr_dist,
                        lr_retain_links, max_tophits, num_clusts_CDS, srp_cutoff, tanglegram_break_segments, max_blk_sz)
    pos, order_links, sr_dist, lr_retain_links, max_tophits = a["pos"], a["order_links"], a["sr_dist"], a["lr_retain_links"], a["max_tophits"]
    num_clusts_CDS, srp_cutoff, tanglegram_break_segments, max_blk_sz = a["num_clusts_CDS"], a["srp_cutoff"], a["tanglegram_break_segments"], a["max_blk_sz"]
    validate_ref_ann_lengths = a["validate_ref_ann_lengths"]
    aln_path = os.path.abspath(aln_path)
    gbk_path, gff3_path, ref_fasta_path = (None if p is None else os.path.abspath(p) for p in (gbk_path, gff3_path, ref_fasta_path))
    dset = str(dset)
    os.makedirs(dset, exist_ok=True)
    log_path = os.path.join(dset, f"LDW_run_{time.strftime('%Y%m%d%H%M%S')}.txt")
    before = set(os.listdir(dset))
    timings = {}
    from .engine import Engine
    own = engine is None
    eng = None
    fh = open(log_path, "w")
    failure = None
    try:
        with contextlib.redirect_stdout(_Tee(fh, sys.stdout if verbose else None)):
            eng = Engine(0) if own else engine
            done = _run(locals(), eng, timings)
    except _Stop as e:
        failure = e
    finally:
        if not fh.closed:
            fh.close()
        if own and eng is not None:
            eng.close()
    if failure is not None:
        raise RuntimeError(str(failure))
    with contextlib.redirect_stdout(sys.stdout if verbose else io.StringIO()):
        moved = cleanup(dset)
    files = {}
    for f in sorted(set(os.listdir(dset)) | set(moved)):
        if f in CLEANUP_FOLDERS or f == "OLD" or (f in before and f not in moved and f not in done):
            continue
        files[f] = moved.get(f, os.path.join(os.path.abspath(dset), f))
    return dict(dset=os.path.abspath(dset), log=files.get(os.path.basename(log_path)), files=files, timings=timings)


class _Stop(Exception):
    """An end of the run that the log must see closed first."""


def _run(v, eng, timings) -> set:
    """Blocks 1-12; ``v``: the driver's normalised arguments and paths.  Returns the names of the top-level entries this run wrote."""
    from . import lr as LR
    from .annotate import perform_snpEff_annotations
    from .cds import estimate_variation_in_CDS, parse_gff_file
    from .extract import parse_fasta_alignment, parse_fasta_SNP_alignment
    from .gbk import parse_genbank_file
    from .mi import estimate_Hamming_distance_weights, perform_MI_computation
    from .network import create_network
    from .output import read_TopHits, write_output_for_gwes_explorer
    from .plots import make_gwes_plots, read_ShortRangeLinks
    from .tanglegram import create_tanglegram
    dset, verbose = v["dset"], v["verbose"]
    gbk_path, gff3_path, sr_only = v["gbk_path"], v["gff3_path"], bool(v["perform_SR_analysis_only"])
    save = bool(v["save_additional_outputs"])
    add_path = os.path.join(dset, "Additional_Outputs")
    at = lambda *names: _first(*[os.path.join(dset, n) for n in names])     # noqa: E731
    snp_path, cds_path, hdw_path = (at(n, os.path.join("Additional_Outputs", n)) for n in ADDITIONAL)
    lr_save_path, sr_save_path = at("lr_links.tsv", os.path.join("Temp", "lr_links.tsv")), at("sr_links.tsv", os.path.join("Temp", "sr_links.tsv"))
    tophits_path = at("sr_tophits.tsv", os.path.join("Tophits", "sr_tophits.tsv"))
    wrote = set()
    t_global = time.time()

    def banner(k):
        print(f"\n\n #################### BLOCK {k} #################### \n")

    def block_done(k, t0):
        timings[f"block_{k}"] = time.time() - t0

    # ---- welcome (:243-275)
    from . import _lib
    print(time.strftime("##------ %a %b %d %H:%M:%S %Y ------##"))
    print(f"\n ***** This is ldweaver_amd (C ABI version {_lib.lib().ldw_version()}) *****")
    print(f"\n\n Performing GWES analysis on: {dset} \n")
    if sr_only:
        print("Only short-range analysis requested. ")
    print(f"All outputs will be saved to: {os.path.abspath(dset)} ")
    print("\n *** Input paths *** \n")
    print(f"* {'Mega Alignment' if v['mega_dset'] else 'Alignment'}: {v['aln_path']} ")
    if v["mega_dset"]:
        print("mega_dset is accepted and ignored: the device path has no separate mode for it ")
    if gbk_path is not None:
        print(f"* GenBank Annotation: {gbk_path} ")
    if gff3_path is not None:
        print(f"* GFF3 Annotation: {gff3_path} ")
    if v["SnpEff_Annotate"]:
        print(f"* Annotations will be performed on short-range links. Annotator: {v['annotator']} ")
    print("\n *** Parameters *** \n")
    if v["snp_filt_method"] == "default":
        print(f"Default SNP filtering: sites with gap_freq < {v['gap_freq']} and non-gap minor allele freq > {v['maf_freq']} will be retained. ")
    else:
        print(f"Relaxed SNP filtering: sites with gap_freq < {v['gap_freq']} and minor allele freq > {v['maf_freq']} will be retained. ")
    print(f"Hamming distance calculation weight: {v['hdw_threshold']} ")
    print(f"Links <= {v['sr_dist']} bp-apart will be classified as short-range (sr-links) ")
    if not sr_only:
        print(f"Approx. top {v['lr_retain_links']:g} long range links will be saved ")
    print(f"Top sr-links with -log10(p) > {v['srp_cutoff']} will be saved ")
    if v["tanglegram_break_segments"] is not None:
        print(f"Tanglegram/GWESExplorer outputs will illustrate upto: {v['max_tophits']} top sr-links ")
    print(f"MI Computation will use a max block size of: {v['max_blk_sz']} x {v['max_blk_sz']} SNPs! Reduce <max_blk_sz> if RAM is scarce!\n")

    # ---- BLOCK 1: the alignment, resident on the engine from here on
    banner(1)
    t0 = time.time()
    fresh_snp = not os.path.exists(snp_path)
    if fresh_snp:
        print(f"Parsing Alignment: {v['aln_path']} ")
        kw = dict(method=v["snp_filt_method"], gap_freq=v["gap_freq"], maf_freq=v["maf_freq"], engine=eng, keep_on_device=True)
        sd = parse_fasta_alignment(v["aln_path"], **kw) if v["aln_has_all_bases"] else parse_fasta_SNP_alignment(v["aln_path"], v["pos"], **kw)
        if save and sd.g is not None:
            os.makedirs(add_path, exist_ok=True)
            print("Step 5: Savings snp.dat...")
            save_snp_dat(snp_path, sd, eng.get_alignment())
            wrote.add(os.path.basename(snp_path))
        print(f"BLOCK 1 complete in {round(time.time() - t0, 2)} s ")
    else:
        print("Loading previous snp matrix ")
        sd = load_snp_dat(snp_path)
        eng.set_alignment(sd.states, max_blk_sz=int(v["max_blk_sz"]))
    block_done(1, t0)

    # ---- BLOCK 2: the annotation (parsed anew in every run: DESIGN.md 25)
    banner(2)
    t0 = time.time()
    gbk = gff = None
    if gbk_path is not None:
        print(f"Reading the GBK file, validate_length_check =  {v['validate_ref_ann_lengths']} ")
        gbk = parse_genbank_file(gbk_path, g=sd.g, length_check=v["validate_ref_ann_lengths"])
    else:
        print("Reading the gff3 file ")
        gff = parse_gff_file(gff3_path, v["ref_fasta_path"], perform_length_check=v["validate_ref_ann_lengths"])
    if sd.g is None:      # a SNP-only alignment takes the genome length from the annotation (:338-345)
        if gbk is not None:
            sd.g = float(gbk["ref_g"])
            print(f"Extracted ref genome length {sd.g:g} from genbank...")
        else:
            sd.g = float(gff.g)
        if save and fresh_snp:
            os.makedirs(add_path, exist_ok=True)
            print("saving snp.dat...")
            save_snp_dat(snp_path, sd, eng.get_alignment())
            wrote.add(os.path.basename(snp_path))
    block_done(2, t0)

    # ---- BLOCK 3
    banner(3)
    t0 = time.time()
    if not os.path.exists(cds_path):
        print("Estimating the variation in CDS ")
        clust_plt_path = os.path.join(dset, "CDS_clustering.png")
        cv = estimate_variation_in_CDS(sd, gbk=gbk, gff=gff, num_clusts_CDS=v["num_clusts_CDS"], clust_plt_path=clust_plt_path, engine=eng,
                                       alignment_resident=True)
        wrote.add("CDS_clustering.png")
        if save:
            save_cds_var(cds_path, cv)
            wrote.add(os.path.basename(cds_path))
    else:
        print("Loading previous CDS variation estimates ")
        cv = load_cds_var(cds_path)
    block_done(3, t0)

    # ---- BLOCK 4
    banner(4)
    t0 = time.time()
    if not os.path.exists(hdw_path):
        print("Estimating per sequence Hamming distance ")
        hdw = estimate_Hamming_distance_weights(sd, threshold=v["hdw_threshold"], engine=eng, alignment_resident=True, verbose=verbose)
        if save:
            np.save(hdw_path, np.asarray(hdw))
            wrote.add(os.path.basename(hdw_path))
    else:
        print("Loading previous Hamming distance estimates ")
        hdw = np.load(hdw_path)
    block_done(4, t0)

    # ---- BLOCK 5
    banner(5)
    t0 = time.time()
    if os.path.exists(sr_save_path) and (sr_only or os.path.exists(lr_save_path)):
        print("Loading previous MI computation ")
        if os.path.getsize(sr_save_path) == 0:      # (an earlier run that kept no link)
            import pandas as pd
            from .plots import SR_COLS
            sr_links = pd.DataFrame({c: np.zeros(0) for c in SR_COLS})
        else:
            sr_links = read_ShortRangeLinks(sr_save_path)
        eng.set_snp_meta(sd.r, sd.uqe, sd.POS, cv.paint, sd.g)      # (the positions the file-fed steps below compare with)
    else:
        print("Commencing MI computation ")
        sr_links = perform_MI_computation(sd, hdw, cv, lr_save_path=lr_save_path, sr_save_path=sr_save_path, plt_folder=dset, sr_dist=v["sr_dist"],
                                          lr_retain_links=v["lr_retain_links"], max_blk_sz=v["max_blk_sz"], srp_cutoff=v["srp_cutoff"], runARACNE=True,
                                          perform_SR_analysis_only=sr_only, order_links=v["order_links"], engine=eng, alignment_resident=True,
                                          verbose=verbose, fit_plots=True)
        wrote.update(["sr_links.tsv"] + ([] if sr_only else ["lr_links.tsv"]))
        wrote.update(f for f in os.listdir(dset) if re.search(r"^c[0-9]+_fit(_data\.tsv|\.png)$", f))
    block_done(5, t0)

    # ---- BLOCK 6
    if not sr_only:
        banner(6)
        t0 = time.time()
        kw = dict(plot_save_path=os.path.join(dset, "LD_plot.png"), plot_title=f"GW-LD: {dset}", lr_links_path=lr_save_path, sr_links_path=sr_save_path,
                  sr_dist=v["sr_dist"])
        try:
            LR.genomewide_LDMap(eng, sd, **kw)
        except _lib.LdwError as e:      # under 1500 positions the default reducer is 1: the reference draws the dense map, the library has none
            if e.code != _lib.LDW_ERR_ARG or "reducer 1 <= 1" not in str(e):
                raise
            print(f"The links hold too few positions for the default reducer: LD map drawn with reducer = {SMALL_LDMAP_REDUCER} ")
            LR.genomewide_LDMap(eng, sd, reducer=SMALL_LDMAP_REDUCER, **kw)
        wrote.add("LD_plot.png")
        block_done(6, t0)
    else:
        print("Genomewide LD map cannot be plotted with only the short_range analysis. If SpydrPick links are avaialble, use genomewide_LDMap()")
    if len(sr_links) == 0:
        raise _Stop(SR_EMPTY)

    # ---- BLOCK 7
    banner(7)
    t0 = time.time()
    make_gwes_plots(lr_links=None, sr_links=sr_links, plt_folder=dset, are_srlinks_ordered=v["order_links"], engine=eng)
    wrote.update(["sr_gwes_clust.png", "sr_gwes_combi.png"])
    block_done(7, t0)

    # ---- BLOCK 8
    banner(8)
    t0 = time.time()
    if v["SnpEff_Annotate"]:
        if not os.path.exists(tophits_path):
            tophits = perform_snpEff_annotations(dset, dset, "snpEff.jar", sd, cv, sr_links,
                                                 gbk=gbk, gbk_path=gbk_path, gff=gff, tophits_path=tophits_path, max_tophits=v["max_tophits"], engine=eng,
                                                 annotator=v["annotator"])
            wrote.update(["sr_snps.vcf", "sr_annotations.tsv", "sr_links_annotated.tsv", "sr_tophits.tsv"])
        else:
            print("Loading previous top hits ")
            tophits = read_TopHits(tophits_path)
        block_done(8, t0)

        # ---- BLOCKS 9-11
        if v["tanglegram_break_segments"] is not None:
            banner(9)
            t0 = time.time()
            folder = os.path.join(dset, "SR_Tanglegram")
            os.makedirs(folder, exist_ok=True)
            create_tanglegram(tophits, gbk=gbk, gff=gff, tanglegram_folder=folder, break_segments=v["tanglegram_break_segments"], engine=eng)
            wrote.add("SR_Tanglegram")
            block_done(9, t0)
        if v["write_gwesExplorer"]:
            banner(10)
            t0 = time.time()
            folder = os.path.join(dset, "SR_GWESExplorer")
            os.makedirs(folder, exist_ok=True)
            write_output_for_gwes_explorer(sd, tophits, folder, engine=eng, alignment_resident=True)
            wrote.add("SR_GWESExplorer")
            block_done(10, t0)
        banner(11)
        t0 = time.time()
        create_network(tophits, netplot_path=os.path.join(dset, "SR_network_plot.png"), plot_title=f"Networks in short-range tophits for {dset}", engine=eng)
        wrote.add("SR_network_plot.png")
        block_done(11, t0)

        # ---- BLOCK 12: the long-range analysis as R/lr_analyser.R:117-181 composes it
        if not sr_only:
            banner(12)
            t0 = time.time()
            if os.path.exists(os.path.join(dset, "lr_tophits.tsv")) or os.path.exists(os.path.join(dset, "Tophits", "lr_tophits.tsv")):
                print("Results from previous LR anlayis exist!")
            else:
                print("Reading long range links... ")
                lr_red = LR.analyse_long_range_links(eng, sd, cds_var=cv, lr_plt_path=os.path.join(dset, "lr_gwes.png"), lr_links_path=lr_save_path,
                                                     sr_links_path=sr_save_path, sr_dist=v["sr_dist"])["lr_links_red"]
                lr_top = perform_snpEff_annotations(dset, dset, "snpEff.jar", sd, cv, lr_red, gbk=gbk, gbk_path=gbk_path, gff=gff,
                                                    tophits_path=os.path.join(dset, "lr_tophits.tsv"), max_tophits=500, links_type="LR", engine=eng,
                                                    annotator=v["annotator"])
                folder = os.path.join(dset, "LR_GWESExplorer")
                os.makedirs(folder, exist_ok=True)
                write_output_for_gwes_explorer(sd, lr_top, folder, links_type="LR", engine=eng, alignment_resident=True)
                create_network(lr_top, netplot_path=os.path.join(dset, "lr_network_plot.png"), plot_title=f"Networks in long-range tophits for {dset}",
                               engine=eng)
                wrote.update(["lr_gwes.png", "lr_snps.vcf", "lr_annotations.tsv", "lr_links_annotated.tsv", "lr_tophits.tsv", "LR_GWESExplorer",
                              "lr_network_plot.png"])
            block_done(12, t0)
    else:
        block_done(8, t0)      # without annotations the run ends here, as the reference's does (:424-428)
    timings["total"] = time.time() - t_global
    print(f"\n\n ** All done in {round(timings['total'] / 60, 3)} m ** ")
    return wrote
