"""GPU: estimate_variation_in_CDS on the device (csrc/ldw_cds.hip through ldw_cds_variation / ldw_cds_paint) against the literal port and the
vectorised twin of tests/cds_ref.py: the golden sample with a synthetic reference, the edges of painter, a bacterial-scale input, and the
pipeline FASTA -> GFF3 -> cds_var -> perform_MI_computation."""
import os
import time
import warnings

import numpy as np
import pandas as pd
import pytest

import cds_ref as R
import ldw_oracle as orc
from ldweaver_amd import _lib as L
from ldweaver_amd import extract
from ldweaver_amd import mi as MIH
from ldweaver_amd.cds import Annotation, estimate_variation_in_CDS, parse_gff_file
from ldweaver_amd.engine import Engine, kmeans_1d
from ldweaver_amd.snpdat import SnpDat
from ldweaver_amd.synth import synth_alignment

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MI_TIGHT = 1e-10


def _mixed_reference(g, rng):
    """Mostly A/C/G/T, with lower case, N, '-' and IUPAC codes mixed in."""
    alpha = np.frombuffer(b"ACGTacgtN-RYKMSW", dtype=np.uint8)
    p = np.array([0.2] * 4 + [0.03] * 4 + [0.02, 0.02] + [0.01] * 6)
    return alpha[rng.choice(len(alpha), size=g, p=p / p.sum())]


def _golden_cds(POS, g, rng, n=40, special=True):
    """Gaps, overlaps, nesting, CDSs without SNPs, boundaries on SNP positions, one end < start (``special=False``: only the first two
    kinds, a CDS without SNPs and one over the last SNPs)."""
    st, en = [], []
    x = 1
    while len(st) < n - 8 and x < g:
        w = int(rng.integers(300, 3000))
        st.append(x)
        en.append(min(g, x + w))
        x += int(rng.integers(-w // 3, w + 2000))      # overlaps (negative step) and gaps
        x = max(x, st[-1] + 1)
    sp = np.sort(POS)
    if special:
        st += [int(sp[100]), int(sp[200]) - 5, int(sp[300])]; en += [int(sp[110]), int(sp[200]) + 5, int(sp[300])]   # on SNPs, a tiny one
        st += [st[2] + 50, st[2] + 60]; en += [en[2] - 50, st[2] + 70]                                              # nested
    gap_lo = int(np.argmax(np.diff(sp)))
    st += [int(sp[gap_lo]) + 1]; en += [int(sp[gap_lo + 1]) - 1]                                                    # no SNP inside
    st += [int(sp[-1]) - 10]; en += [g]                                                                              # covers the last SNPs
    if special:
        st += [500]; en += [400]                                                                                     # end < start
    return np.array(st, dtype=np.int64), np.array(en, dtype=np.int64)


def _kmeans_cluster(x, k):
    lab, _ = kmeans_1d(np.asarray(x, dtype=np.float64), k)
    return R.clusters_by_mean(lab, x)


def _run(engine, sd, ann, k, quirk):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        cv = estimate_variation_in_CDS(sd, gff=ann, num_clusts_CDS=k, engine=engine, alignment_resident=True, quirk_mode=quirk)
    return cv, [x for x in w if issubclass(x.category, UserWarning)]


def _compare_literal(cv, lit):
    assert np.array_equal(cv.var_estimate, lit["var_estimate"])          # bit-identical, same NA drop
    assert np.array_equal(cv.cds_start, lit["cds_start"]) and np.array_equal(cv.cds_end, lit["cds_end"])
    assert np.array_equal(cv.clusts["km_clst_ord"], lit["km_clst_ord"]) and cv.clusts["cutoff"] == lit["cutoff"]
    assert cv.ref.tolist() == lit["ref"] and cv.alt == lit["alt"]
    assert np.array_equal(cv.paint, lit["paint"])


def test_golden_sample(engine, sample):
    rng = np.random.default_rng(41)
    st, POS, g = sample["states"], sample["POS"], 50000
    ref = _mixed_reference(g, rng)
    starts, ends = _golden_cds(POS, g, rng)
    ann = Annotation.from_arrays(starts, ends, ref)
    sd = SnpDat.from_states(st, POS, float(g))
    engine.set_alignment(st)
    counts = orc.acgtn_table(st)
    for quirk in (L.QUIRK_REFERENCE, L.QUIRK_INTENDED):
        cv, warned = _run(engine, sd, ann, 3, quirk)
        assert np.array_equal(cv.allele_table, engine.state_counts()) and np.array_equal(cv.allele_table, counts)
        lit = R.estimate_literal(list(POS), counts, bytes(ref), list(starts), list(ends), 3, _kmeans_cluster, quirk)
        _compare_literal(cv, lit)
        assert np.isnan(lit["var_all"]).sum() >= 2 and len(cv.var_estimate) >= 20
        assert 0 not in cv.paint.tolist() and not warned
        assert sum(c.islower() for c in cv.ref) > 0 and sum(c in "N-" for c in cv.ref) > 0 and sum(c in "RYKMSW" for c in cv.ref) > 0


def _small(engine, POS, starts, ends, k=2, quirk=L.QUIRK_REFERENCE, N=7, seed=0, g=None):
    rng = np.random.default_rng(seed)
    POS = np.asarray(POS, dtype=np.int64)
    g = g or int(max(POS.max(), np.max(ends) if len(ends) else 1)) + 5
    st = rng.integers(0, 5, size=(len(POS), N)).astype(np.uint8)
    ref = _mixed_reference(g, rng)
    engine.set_alignment(st)
    sd = SnpDat.from_states(st, POS.astype(np.int32), float(g))
    ann = Annotation.from_arrays(starts, ends, ref)
    counts = orc.acgtn_table(st)
    try:
        lit = R.estimate_literal(list(POS), counts, bytes(ref), list(starts), list(ends), k, _kmeans_cluster, quirk)
    except ValueError as e:
        lit = e
    try:
        cv, warned = _run(engine, sd, ann, k, quirk)
    except ValueError as e:
        cv, warned = e, []
    return cv, lit, warned


def _ok(cv, lit):
    assert not isinstance(cv, Exception) and not isinstance(lit, Exception), (cv, lit)
    _compare_literal(cv, lit)


def test_edges_order_and_sizes(engine):
    # unsorted, repeated positions (one repeat on a CDS boundary)
    cv, lit, _ = _small(engine, [50, 12, 30, 30, 7, 90, 12, 61, 44, 44, 3, 77], [5, 25, 40, 70], [35, 45, 80, 95])
    _ok(cv, lit)
    # L = 1 (the reference stops at 2:1): the paint as it stands
    cv, lit, _ = _small(engine, [20], [10], [30], k=1)
    _ok(cv, lit)
    assert cv.paint.tolist() == [1]
    # ncds = 1
    cv, lit, _ = _small(engine, [5, 9, 14, 20, 26], [4], [30], k=1)
    _ok(cv, lit)
    assert cv.paint.tolist() == [1] * 5
    # no interior 0 run (the reference stops at 1:length(rm0s)): leading and trailing runs filled, nothing else
    cv, lit, _ = _small(engine, [2, 5, 9, 14, 20, 26, 40, 41], [4, 12], [15, 30], k=2)
    _ok(cv, lit)
    assert 0 not in cv.paint.tolist()


def test_edges_trailing_single_snp(engine):
    POS, starts, ends = [5, 9, 14, 20, 26, 33, 60], [4, 18], [15, 40]
    cv, lit, warned = _small(engine, POS, starts, ends, k=2, quirk=L.QUIRK_REFERENCE)
    _ok(cv, lit)
    assert cv.paint[-1] == 0 and 0 not in cv.paint[:-1].tolist()
    assert len(warned) == 1 and "SNP 6 (POS 60)" in str(warned[0].message) and "QUIRK_INTENDED" in str(warned[0].message)
    cv, lit, warned = _small(engine, POS, starts, ends, k=2, quirk=L.QUIRK_INTENDED)
    _ok(cv, lit)
    assert cv.paint[-1] == cv.paint[-2] != 0 and not warned
    # a painted single last SNP is kept, a 0 run before it is the last recorded run and takes the left value
    cv, lit, _ = _small(engine, [5, 9, 14, 20, 26, 33, 60], [4, 55], [15, 70], k=2)
    _ok(cv, lit)


def test_edges_unpainted_and_nclust(engine):
    # every SNP on a CDS boundary or outside: no SNP strictly inside
    cv, lit, _ = _small(engine, [5, 9, 14], [5, 9], [9, 14], k=1)
    assert isinstance(cv, ValueError) and isinstance(lit, ValueError)
    # only the unrecorded last SNP is painted (reference mode): the reference stops at region_mat[1, 2]
    cv, lit, _ = _small(engine, [5, 9, 14, 20], [15], [30], k=1)
    assert isinstance(cv, ValueError) and isinstance(lit, ValueError)
    cv, lit, _ = _small(engine, [5, 9, 14, 20], [15], [30], k=1, quirk=L.QUIRK_INTENDED)
    _ok(cv, lit)
    rng = np.random.default_rng(8)
    POS = np.sort(rng.choice(np.arange(1, 3000), size=400, replace=False))
    starts = np.sort(rng.choice(np.arange(1, 2900), size=60, replace=False))
    ends = starts + rng.integers(5, 120, size=60)
    for k in (1, 3, 8):
        for quirk in (L.QUIRK_REFERENCE, L.QUIRK_INTENDED):
            cv, lit, _ = _small(engine, POS, starts, ends, k=k, quirk=quirk, N=23, seed=k)
            _ok(cv, lit)
            assert set(cv.clusts["km_clst_ord"].tolist()) == set(range(1, k + 1))


def test_abi_errors(engine):
    with Engine(0) as fresh:
        with pytest.raises(L.LdwError) as e:
            fresh.cds_variation([1, 2], b"ACGT", [1], [3])
        assert e.value.code == L.LDW_ERR_STATE and "no alignment resident" in str(e.value)
        with pytest.raises(L.LdwError) as e:
            fresh.cds_paint([1], [3], [1], 1)
        assert e.value.code == L.LDW_ERR_STATE
    st = np.zeros((3, 4), dtype=np.uint8)
    engine.set_alignment(st)
    for POS, msg in (([1, 2, 9], "outside 1..8"), ([0, 2, 3], "outside 1..8"), ([1, 2], "resident alignment has 3")):
        with pytest.raises(L.LdwError) as e:
            engine.cds_variation(POS, b"ACGTACGT", [1], [3])
        assert e.value.code == L.LDW_ERR_ARG and msg in str(e.value)
    var, snp_var, alt, refc = engine.cds_variation([1, 2, 8], b"ACGTACGt", [1, 5, 3], [3, 7, 2])
    assert np.isnan(var[1]) and np.isnan(var[2]) and var[0] == 4 / 3 and snp_var.tolist() == [0, 4, 4] and bytes(refc) == b"ACt"
    for args in (([1], [3], [2], 1), ([1], [3], [0], 1), ([1], [3], [1], 0), ([1], [3], [1], 256)):
        with pytest.raises(L.LdwError) as e:
            engine.cds_paint(*args)
        assert e.value.code == L.LDW_ERR_ARG
    with pytest.raises(L.LdwError) as e:
        engine.cds_paint([1], [3], [1], 1, quirk_mode=2)
    assert e.value.code == L.LDW_ERR_ARG
    with pytest.raises(ValueError, match="no SNP lies strictly inside"):
        engine.cds_paint([1], [2], [1], 1)


def test_scale_bacterial_genome(engine):
    """L = 500 000 SNPs over 2.2 Mb (synth.py's recipe), ~5 000 CDSs: exactly the vectorised twin; the device calls are timed."""
    g = 2_200_000
    syn = synth_alignment(L=500_000, N=24, seed=11, g=g)
    st, POS = syn["states"], syn["POS"]
    rng = np.random.default_rng(12)
    ref = _mixed_reference(g, rng)
    starts = np.sort(rng.integers(1, g - 3000, size=5000))
    ends = starts + rng.integers(-5, 2500, size=5000)
    engine.set_alignment(st)
    counts = engine.state_counts()
    for quirk in (L.QUIRK_REFERENCE, L.QUIRK_INTENDED):
        t0 = time.perf_counter()
        var, snp_var, alt, refc = engine.cds_variation(POS, ref, starts, ends)
        t1 = time.perf_counter()
        wv, wsv, walt, wref = R.variation_vec(POS, counts, ref, starts, ends)
        assert np.array_equal(var, wv, equal_nan=True) and np.array_equal(snp_var, wsv) and np.array_equal(alt, walt) and np.array_equal(refc, wref)
        keep = ~np.isnan(var)
        lab, _ = kmeans_1d(var[keep], 3)
        t2 = time.perf_counter()
        paint, n0 = engine.cds_paint(starts[keep], ends[keep], lab, 3, quirk)
        t3 = time.perf_counter()
        wp, wn0 = R.paint_vec(POS, starts[keep], ends[keep], lab, quirk)
        assert np.array_equal(paint, wp) and n0 == wn0
        print(f"\nL = 500000, ncds = 5000, quirk {quirk}: ldw_cds_variation {1e3 * (t1 - t0):.2f} ms, ldw_cds_paint {1e3 * (t3 - t2):.2f} ms (wall)")


def _write_fasta(path, name, seq: bytes, width=60):
    with open(path, "wb") as fh:
        fh.write(b">" + name + b" reference\n")
        for i in range(0, len(seq), width):
            fh.write(seq[i:i + width] + b"\n")


def test_pipeline_fasta_gff_cds_var_mi(engine, tmp_path):
    pos = np.loadtxt(os.path.join(GOLDEN, "snp_sample.pos"), dtype=np.int64)
    sd = extract.parse_fasta_SNP_alignment(os.path.join(GOLDEN, "snp_sample.fa.gz"), pos, engine=engine)
    assert sd.g is None
    rng = np.random.default_rng(77)
    g = 50000
    ref = _mixed_reference(g, rng)
    starts, ends = _golden_cds(sd.POS, g, rng, special=False)
    keep = ends >= starts
    lines = ["##gff-version 3", "# written by the test"]
    for j, (s, e) in enumerate(zip(starts[keep], ends[keep])):
        lines.append(f"ref1\ttest\t{'CDS' if j % 3 else 'cds'}\t{s}\t{e}\t.\t+\t0\tID=cds{j}")
        if j % 5 == 0:
            lines.append(f"ref1\ttest\tgene\t{s}\t{e}\t.\t+\t.\tID=gene{j}")
    (tmp_path / "a.gff3").write_text("\r\n".join(lines) + "\r\n##FASTA\n>ref1\nACGT\n")
    _write_fasta(tmp_path / "ref.fa", b"ref1", bytes(ref))
    ann = parse_gff_file(str(tmp_path / "a.gff3"), str(tmp_path / "ref.fa"))
    assert ann.g == g and ann.ref_name == "ref1"
    sd.g = float(ann.g)                            # R/BacGWES.R:338-345
    cv = estimate_variation_in_CDS(sd, gff=ann, engine=engine, alignment_resident=True)
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
