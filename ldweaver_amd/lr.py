"""Consumers of the link tables (SURVEY.md §8 f rank 4): the numeric cores of ``analyse_long_range_links``
(R/lr_analyser.R:29-190) and ``genomewide_LDMap`` (R/LDSummaryPlot.R:25-125) on the device-resident tables of the
engine.  Plots, SnpEff annotation and the tanglegram are out of scope (SURVEY.md §8 f)."""
from __future__ import annotations

import warnings

import numpy as np
import pandas as pd

from .rcompat import circ_len


SR_TSV_COLS = ["clust_c", "pos1", "pos2", "clust1", "clust2", "len", "MI", "srp_max", "ARACNE"]   # R/computePairwiseMI.R:140


def positions_to_snp_index(POS, p) -> np.ndarray:
    """0-based SNP index of every position in ``p`` — ``snp.dat$POS`` in ANY order (the reference imposes none: R/computePairwiseMI.R:176-177;
    r03 assumed ascending positions here); a position held by several SNPs maps to the first of them.  Raises on a position that is no SNP's."""
    POS = np.asarray(POS)
    p = np.asarray(p)
    order = np.argsort(POS, kind="stable")
    srt = POS[order]
    k = np.searchsorted(srt, p, side="left")
    if len(p) and not np.array_equal(srt[np.minimum(k, len(srt) - 1)], p):
        raise ValueError("sr_links holds positions that are not SNP positions of snp_dat")
    return order[np.minimum(k, len(srt) - 1)] if len(p) else np.zeros(0, dtype=np.int64)


def _int32_positions(cols):
    """Sorted distinct values of device position columns that are int32 integers (the others are left for ldw_links_load to refuse, with their line)."""
    import torch
    p = torch.cat([c for c in cols])
    p = p[(p == torch.floor(p)) & (p.abs() < 2.0 ** 31)]
    return torch.unique(p).cpu().numpy().astype(np.int32)


def load_link_files(eng, snp_dat=None, lr_links_path=None, sr_links_path=None, links_from_spydrpick: bool = False, sr_dist=20000, g=None,
                    load_sr: bool = True) -> dict:
    """The engine's link tables from files (ldw_tsv_read + ldw_links_load): lr_links.tsv or a SpydrPick file becomes the long-range table (rows
    with len < sr_dist dropped), sr_links.tsv the short-range one (``load_sr``; with ``snp_dat=None`` that file is parsed twice, once for its positions and once into the table: the engine has one
    column buffer).  Positions: those of ``snp_dat`` — an engine that holds its
    alignment keeps it, a fresh one takes POS and g alone (ldw_set_positions) — or, with ``snp_dat=None``, the sorted distinct positions of the
    files.  Returns what the callers need of the files beside the tables: ``lr`` (device columns by name, aliases of the engine's buffer), ``lr_rows``
    (file row of every long-range table row, device), ``sr`` (the short-range frame or None), ``POS``."""
    import torch
    from .links_io import read_links_native, table_shape
    if lr_links_path is None:
        raise ValueError("lr_links_path is needed: the long-range table comes from the file")
    sr, sr_pos = None, []
    if sr_links_path is not None and not load_sr:      # the caller wants the rows on the host (ldw_lr_tukey takes them from there)
        sr = read_links_native(sr_links_path, "sr", engine=eng)
    elif sr_links_path is not None and snp_dat is None:   # only its positions, for POS: kept on the device while the long-range file is read
        eng.tsv_read(sr_links_path, "\t", len(SR_TSV_COLS))
        c = eng.tsv_columns()
        sr_pos = [c[SR_TSV_COLS.index("pos1")].clone(), c[SR_TSV_COLS.index("pos2")].clone()]
        torch.cuda.current_stream().synchronize()
    kind = "spydrpick" if links_from_spydrpick else "lr"
    sep, names = table_shape(lr_links_path, kind)
    rows, _, _ = eng.tsv_read(lr_links_path, sep, len(names))
    lr = dict(zip(names, eng.tsv_columns()))
    keep = ~(lr["len"] < float(sr_dist)) if rows else torch.zeros(0, dtype=torch.bool, device=torch.device("cuda", eng.device))
    if snp_dat is None:
        cols = [lr["pos1"][keep], lr["pos2"][keep]] + sr_pos
        if sr is not None:
            dev = cols[0].device
            cols += [torch.as_tensor(sr[k].to_numpy(dtype=np.float64), device=dev) for k in ("pos1", "pos2")]
        POS = _int32_positions(cols)
        if len(POS) == 0:
            raise ValueError("the link files hold no positions")
        eng.set_positions(POS, 0.0 if g is None else float(g))
    else:
        POS = np.asarray(snp_dat.POS)
        have = getattr(eng, "_positions", None)
        if have is None:
            if eng.N > 0:
                raise ValueError("the engine holds an alignment whose positions were not set through Engine.set_snp_meta: they cannot be compared with "
                                 "snp_dat.POS, and ldw_set_positions would drop the alignment (use a fresh Engine)")
            eng.set_positions(POS, float(snp_dat.g if g is None else g))
        elif not np.array_equal(have, POS):
            raise ValueError("snp_dat.POS differs from the positions the engine holds (use a fresh Engine: new positions would drop its alignment and tables)")
    torch.cuda.current_stream().synchronize()   # (the library works on its own stream: torch's reads of the columns above are done)
    eng.links_load(1, names.index("pos1"), names.index("pos2"), names.index("MI"), names.index("len"), float(sr_dist))
    lr_rows = torch.nonzero(keep).reshape(-1)
    if load_sr:
        if sr_links_path is None:
            eng.links_import(0, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0))
        else:   # (the one buffer holds the long-range columns: what the caller needs of them is copied first)
            lr = {k: v.clone() for k, v in lr.items()}
            torch.cuda.current_stream().synchronize()
            eng.tsv_read(sr_links_path, "\t", len(SR_TSV_COLS))
            eng.links_load(0, SR_TSV_COLS.index("pos1"), SR_TSV_COLS.index("pos2"), SR_TSV_COLS.index("MI"))
    return dict(lr=lr, lr_rows=lr_rows, sr=sr, POS=POS, names=names)


def _analyse_from_files(eng, snp_dat, cds_var, are_lrlinks_ordered, min_links, lr_plt_path, lr_links_path, sr_links_path, links_from_spydrpick, sr_dist, g):
    import torch
    t = load_link_files(eng, snp_dat, lr_links_path, sr_links_path, links_from_spydrpick, sr_dist, g, load_sr=False)
    POS, lr, sr = t["POS"], t["lr"], t["sr"]
    srt = None
    if sr is not None:
        sb_, sa_ = positions_to_snp_index(POS, sr["pos1"].to_numpy()), positions_to_snp_index(POS, sr["pos2"].to_numpy())
        srt = (sa_, sb_, sr["MI"].to_numpy(dtype=np.float64))
    info = eng.lr_tukey(min_links, sr=srt)
    if info["fallback"]:   # R/lr_analyser.R:96
        warnings.warn("Not enough lr links pass the Tukey criteria, ~5000 top links were retained instead")
    red = eng.lr_reduced()
    file_rows = t["lr_rows"][torch.as_tensor(red["row"], device=t["lr_rows"].device)]
    if "ARACNE" in lr:     # a SpydrPick file with its own flags: ARACNE is not run again (R/lr_analyser.R:101)
        flags = lr["ARACNE"][file_rows].cpu().numpy() != 0
    else:
        flags = eng.aracne_device()
    if lr_plt_path is not None:   # len as the file has it, straight from the device columns
        from . import plots
        plots.render_scatter(eng, lr["len"][file_rows], lr["MI"][file_rows], None, torch.as_tensor(flags.astype(np.uint8), device=file_rows.device),
                             opts=plots.plot_opts(plots.L.PLOT_LR, layer_rgb=(plots.GREY, plots.LR_DIRECT), hline=float(np.max(info["thresholds"]))),
                             path=lr_plt_path)
    a, b = red["a"], red["b"]
    cols = dict(pos1=POS[b].astype(np.int64), pos2=POS[a].astype(np.int64))     # to side = pos1, from side = pos2 (R/computePairwiseMI.R:319-320)
    if cds_var is not None:
        paint = np.asarray(cds_var.paint)
        cols.update(clust1=paint[b], clust2=paint[a])
    elif "c1" in lr:
        cols.update(clust1=lr["c1"][file_rows].cpu().numpy(), clust2=lr["c2"][file_rows].cpu().numpy())
    cols.update(len=lr["len"][file_rows].cpu().numpy(), MI=red["MI"], ARACNE=flags.astype(int))
    df = pd.DataFrame(cols)
    if not are_lrlinks_ordered:    # :115-117
        df = df.iloc[np.argsort(-df["MI"].to_numpy(), kind="stable")].reset_index(drop=True)
    return dict(lr_links_red=df, q13=info["q13"], thresholds=info["thresholds"], fallback=info["fallback"], n_pool=info["n_pool"])


def analyse_long_range_links(eng, snp_dat=None, sr_links=None, cds_var=None, are_lrlinks_ordered: bool = False, min_links: int = 5000,
                             lr_plt_path=None, *, lr_links_path=None, sr_links_path=None, links_from_spydrpick: bool = False, sr_dist=20000,
                             g=None) -> dict:
    """Tukey outlier analysis + ARACNE of the long-range links the engine holds after ``perform_MI_computation`` /
    ``mi_all_pairs`` (the reference reads them back from lr_links.tsv).  ``sr_links`` is the short-range part of the ARACNE
    pool exactly as the reference has it: the contents of sr_links.tsv (R/lr_analyser.R:67), i.e. the REDUCED frame
    ``perform_MI_computation`` returned (srp_max > srp_cutoff) — pass that frame (pos1, pos2, MI columns) or the path of the
    tsv.  Returns the reference's ``lr_links_red`` (pos1 pos2 [clust1 clust2] len MI ARACNE, descending MI unless
    ``are_lrlinks_ordered``) plus the thresholds.  Everything O(#links) runs on the device (ldw_lr_tukey, ldw_aracne_device).
    ``lr_plt_path``: also write the reference's ``lr_gwes.png`` there (R/lr_analyser.R:117-127: indirect links grey under the direct ones, a
    line at max(thresholds)), rendered from the outlier links while they are resident (ldw_plot_links).
    ``lr_links_path`` (with ``sr_links_path``, ``links_from_spydrpick``, ``sr_dist``): the reference's file inputs — the long-range links come from
    lr_links.tsv or a SpydrPick file through the native reader (load_link_files), ``len`` is the file's, and a SpydrPick file with an ARACNE column
    keeps its flags (R/lr_analyser.R:101).  Then ``snp_dat`` may be None: the engine needs no alignment, the positions are those of the files, and
    ``g`` is not needed."""
    if lr_links_path is not None:
        if sr_links is not None:
            raise ValueError("with lr_links_path the short-range links come from sr_links_path, not sr_links")
        return _analyse_from_files(eng, snp_dat, cds_var, are_lrlinks_ordered, min_links, lr_plt_path, lr_links_path, sr_links_path, links_from_spydrpick,
                                   sr_dist, g)
    if sr_links_path is not None or links_from_spydrpick:
        raise ValueError("sr_links_path and links_from_spydrpick go with lr_links_path")
    if snp_dat is None or sr_links is None:
        raise ValueError("without lr_links_path, snp_dat and sr_links are needed: the long-range links are those the engine holds")
    if isinstance(sr_links, (str, bytes)) or hasattr(sr_links, "__fspath__"):
        sr_links = pd.read_csv(sr_links, sep="\t", header=None, names=SR_TSV_COLS)
    POS_ = np.asarray(snp_dat.POS)
    p1, p2 = np.asarray(sr_links["pos1"]), np.asarray(sr_links["pos2"])
    sb_, sa_ = positions_to_snp_index(POS_, p1), positions_to_snp_index(POS_, p2)      # pos1 = to side (b), pos2 = from side (a)
    info = eng.lr_tukey(min_links, sr=(sa_, sb_, np.asarray(sr_links["MI"], dtype=np.float64)))
    if info["fallback"]:   # R/lr_analyser.R:96
        warnings.warn("Not enough lr links pass the Tukey criteria, ~5000 top links were retained instead")
    red = eng.lr_reduced()
    flags = eng.aracne_device()
    if lr_plt_path is not None:
        from . import plots
        plots.render_links(eng, 1, opts=plots.plot_opts(plots.L.PLOT_LR, layer_rgb=(plots.GREY, plots.LR_DIRECT), hline=float(np.max(info["thresholds"]))),
                           use_aracne=len(flags) > 0, path=lr_plt_path)
    POS = np.asarray(snp_dat.POS)
    a, b = red["a"], red["b"]
    pos1, pos2 = POS[b].astype(np.int64), POS[a].astype(np.int64)     # to side = pos1, from side = pos2 (R/computePairwiseMI.R:319-320)
    cols = dict(pos1=pos1, pos2=pos2)
    if cds_var is not None:
        paint = np.asarray(cds_var.paint)
        cols.update(clust1=paint[b], clust2=paint[a])
    cols.update(len=circ_len(pos1.astype(float), pos2.astype(float), float(snp_dat.g)), MI=red["MI"], ARACNE=flags.astype(int))
    df = pd.DataFrame(cols)
    if not are_lrlinks_ordered:    # :115-117
        df = df.iloc[np.argsort(-df["MI"].to_numpy(), kind="stable")].reset_index(drop=True)
    return dict(lr_links_red=df, q13=info["q13"], thresholds=info["thresholds"], fallback=info["fallback"], n_pool=info["n_pool"])


def genomewide_LDMap(eng, snp_dat=None, reducer=None, from_=None, to=None, plot_save_path=None, plot_title=None, *, lr_links_path=None,
                     sr_links_path=None, links_from_spydrpick: bool = False, sr_dist=20000) -> dict:
    """Numeric core of ``genomewide_LDMap``: the reduced, log10-scaled, 0..1-rescaled LD matrix ``htm`` with its row /
    column labels (the reference's ``nms``: pos_vec[seq(1, n, by = reducer - 1)][1:B], R/LDSummaryPlot.R:95-96).
    ``plot_save_path``: also write the reference's ``LD_plot.png`` there (R/LDSummaryPlot.R:121-128), rendered from the map's device copy
    (ldw_plot_ldmap), under ``plot_title``.
    ``lr_links_path`` / ``sr_links_path`` (``links_from_spydrpick``, ``sr_dist``): the tables come from the files instead (load_link_files); with
    ``snp_dat=None`` the engine needs no alignment and the positions are those of the files."""
    if lr_links_path is not None:
        load_link_files(eng, snp_dat, lr_links_path, sr_links_path, links_from_spydrpick, sr_dist)
    elif sr_links_path is not None or links_from_spydrpick:
        raise ValueError("sr_links_path and links_from_spydrpick go with lr_links_path")
    if reducer is not None and reducer < 0:     # :30-35
        warnings.warn("<reducer> for genomewide_LDMap should be >0, set to default")
        reducer = None
    if (from_ is None) != (to is None):         # :37-38
        raise ValueError("If <from> is provided, <to> must be provided as well!" if to is None else
                         "If <to> is provided, <from> must be provided as well!")
    if from_ is not None:                       # :43-47
        if to <= from_:
            raise ValueError("<to> must be greater than <from>!")
        if from_ < 0 or to < 0:
            raise ValueError("<from> and <to> must be positive values")
        from_, to = int(round(from_)), int(round(to))
    r = 0 if reducer is None else int(np.round(reducer))
    if plot_save_path is None:
        htm, n_pos, r = eng.ldmap(r, from_ or 0, to or 0)
    else:
        htm, n_pos, r = eng.ldmap(r, from_ or 0, to or 0, plot_save_path=plot_save_path, plot_title=plot_title)
    return dict(htm=htm, n_pos=n_pos, reducer=r)
