"""CPU: the CDS variation / paint restatements against each other, the host k-means against brute force and Lloyd, the GFF3 and reference
FASTA readers, and the extended CdsVar (ldweaver_amd.cds; R/estimateCDSDiversity.R, R/parseGFF.R)."""
import gzip
import itertools

import numpy as np
import pytest

import cds_ref as R
from ldweaver_amd import cds
from ldweaver_amd.engine import kmeans_1d
from ldweaver_amd.snpdat import CdsVar

REF_ALPHABET = np.frombuffer(b"ACGTACGTACGTNacgtn-RYKM", dtype=np.uint8)


def _kmeans_cluster(x, k):
    lab, _ = kmeans_1d(np.asarray(x, dtype=np.float64), k)
    return R.clusters_by_mean(lab, x)


def _random_case(rng):
    g = int(rng.integers(8, 70))
    L = int(rng.integers(1, 30))
    N = int(rng.integers(1, 7))
    kind = rng.integers(0, 3)
    if kind == 0:
        POS = np.sort(rng.choice(np.arange(1, g + 1), size=min(L, g), replace=False))
    elif kind == 1:
        POS = np.sort(rng.integers(1, g + 1, size=L))      # repeated positions
    else:
        POS = rng.integers(1, g + 1, size=L)               # any order, repeats
    L = len(POS)
    states = rng.integers(0, 5, size=(L, N))
    counts = np.stack([(states == x).sum(axis=1) for x in range(5)])
    ref = REF_ALPHABET[rng.integers(0, len(REF_ALPHABET), size=g)]
    ncds = int(rng.integers(1, 9))
    starts = rng.integers(0, g + 1, size=ncds)
    ends = starts + rng.integers(-2, g // 2 + 2, size=ncds)
    if ncds > 1 and rng.random() < 0.3:            # a CDS nested in another
        ends[1] = ends[0] - 1
        starts[1] = starts[0] + 1
    # boundaries exactly on SNP positions
    for j in range(ncds):
        if rng.random() < 0.3:
            starts[j] = POS[rng.integers(0, L)]
        if rng.random() < 0.3:
            ends[j] = POS[rng.integers(0, L)]
    k = int(rng.integers(1, 4))
    return dict(POS=POS.astype(np.int64), counts=counts, ref=ref, starts=starts.astype(np.int64), ends=ends.astype(np.int64), k=k)


def _vec(case, quirk):
    var, snp_var, alt, refc = R.variation_vec(case["POS"], case["counts"], case["ref"], case["starts"], case["ends"])
    keep = ~np.isnan(var)
    ve, cs, ce = var[keep], case["starts"][keep], case["ends"][keep]
    lab, cutoff = kmeans_1d(ve, case["k"])
    paint, n0 = R.paint_vec(case["POS"], cs, ce, lab, quirk)
    return dict(var_all=var, var_estimate=ve, cds_start=cs, cds_end=ce, km_clst_ord=lab, cutoff=cutoff, paint=paint, n0=n0,
                alt=R.alt_strings(alt), ref=[chr(c) for c in refc], snp_var=snp_var)


def _outcome(fn):
    try:
        return fn()
    except ValueError as e:
        return ("ValueError", "distinct" in str(e))


def test_literal_equals_vectorised_on_random_cases():
    """~2 000 seeded small cases: the literal port (region_mat, R's round) and the vectorised twin agree on every output, in both quirk modes,
    and the cases reach every branch of painter named in the contract."""
    rng = np.random.default_rng(20261016)
    seen = dict(leading=0, trailing=0, interior_odd=0, interior_even=0, interior_single=0, dropped=0, dropped_zero=0, nested=0, repeated=0,
                unsorted=0, no_interior=0, single=0, value_error=0, cds_without_snp=0)
    n_cases = 0
    while n_cases < 2000:
        case = _random_case(rng)
        n_cases += 1
        POS = case["POS"]
        seen["repeated"] += len(np.unique(POS)) < len(POS)
        seen["unsorted"] += bool(np.any(np.diff(POS) < 0))
        seen["single"] += len(POS) == 1
        for quirk in (R.QUIRK_REFERENCE, R.QUIRK_INTENDED):
            lit = _outcome(lambda: R.estimate_literal(list(POS), case["counts"], bytes(case["ref"]), list(case["starts"]), list(case["ends"]),
                                                      case["k"], _kmeans_cluster, quirk))
            vec = _outcome(lambda: _vec(case, quirk))
            if isinstance(lit, tuple) or isinstance(vec, tuple):
                assert lit == vec, (n_cases, quirk, lit if isinstance(lit, tuple) else "ok", vec if isinstance(vec, tuple) else "ok")
                seen["value_error"] += 1
                continue
            assert np.array_equal(lit["var_all"], vec["var_all"], equal_nan=True), n_cases
            assert np.array_equal(lit["snp_var"], vec["snp_var"]) and lit["alt"] == vec["alt"] and lit["ref"] == vec["ref"]
            for f in ("var_estimate", "cds_start", "cds_end", "km_clst_ord", "paint"):
                assert np.array_equal(lit[f], vec[f]), (n_cases, quirk, f, lit[f], vec[f])
            assert lit["cutoff"] == vec["cutoff"]
            seen["cds_without_snp"] += bool(np.isnan(lit["var_all"]).any())
            if quirk == R.QUIRK_REFERENCE:
                # which painter branches this case took (from the stabbed paint)
                vs = _vec(case, quirk)
                lab = vs["km_clst_ord"]
                order = np.argsort(POS, kind="stable")
                p = np.zeros(len(POS), dtype=np.int32)
                for j in range(len(lab)):
                    inside = (vs["cds_start"][j] < POS) & (POS < vs["cds_end"][j])
                    p[inside] = np.maximum(p[inside], lab[j])
                del order
                if len(p) > 1:
                    runs = [(k, len(list(gr))) for k, gr in itertools.groupby(p.tolist())]
                    dropped = runs[-1][1] == 1 and len(runs) > 1
                    seen["dropped"] += dropped
                    seen["dropped_zero"] += dropped and runs[-1][0] == 0
                    seen["leading"] += runs[0][0] == 0
                    rec = runs[:-1] if dropped else runs
                    seen["trailing"] += rec[-1][0] == 0
                    inner = [ln for v, ln in rec[1:-1] if v == 0]
                    seen["no_interior"] += not inner
                    seen["interior_single"] += any(ln == 1 for ln in inner)
                    seen["interior_odd"] += any(ln > 1 and (ln - 1) % 2 == 1 for ln in inner)
                    seen["interior_even"] += any(ln > 1 and (ln - 1) % 2 == 0 for ln in inner)
                st, en = vs["cds_start"], vs["cds_end"]
                seen["nested"] += any(st[a] < st[b] and en[b] < en[a] for a in range(len(st)) for b in range(len(st)))
                assert vec["n0"] == int(dropped and runs[-1][0] == 0) if len(p) > 1 else True
            else:
                assert vec["n0"] == 0
    for k, v in seen.items():
        assert v >= 20, (k, seen)


def test_round_half_even():
    assert [R.r_round(x / 2) for x in range(1, 10)] == [0, 1, 2, 2, 2, 3, 4, 4, 4]
    assert [R.r_round(x / 2) for x in range(1, 10)] == [int(np.round(x / 2)) for x in range(1, 10)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# k-means
# ---------------------------------------------------------------------------------------------------------------------------------------
def _sse(x, groups):
    return sum(float(((x[g] - x[g].mean()) ** 2).sum()) for g in groups if len(g))


def _brute(x, k):
    """Every partition of the sorted distinct values into k contiguous groups: (best cost, list of optimal partitions as value bounds)."""
    u = np.unique(x)
    best, arg = None, []
    for cuts in itertools.combinations(range(1, len(u)), k - 1):
        b = (0,) + cuts + (len(u),)
        groups = [np.flatnonzero((x >= u[b[q]]) & (x <= u[b[q + 1] - 1])) for q in range(k)]
        c = _sse(x, groups)
        if best is None or c < best * (1 - 1e-13) - 1e-300:
            best, arg = c, [b]
        elif c <= best * (1 + 1e-13) + 1e-300:
            arg.append(b)
    return best, arg, u


def _lloyd(x, k, rng, iters=100):
    c = rng.choice(np.unique(x), size=k, replace=False)
    for _ in range(iters):
        a = np.argmin(np.abs(x[:, None] - c[None, :]), axis=1)
        nc = np.array([x[a == q].mean() if np.any(a == q) else c[q] for q in range(k)])
        if np.array_equal(nc, c):
            break
        c = nc
    a = np.argmin(np.abs(x[:, None] - c[None, :]), axis=1)
    return _sse(x, [np.flatnonzero(a == q) for q in range(k)])


@pytest.mark.parametrize("seed", range(12))
def test_kmeans_exact_against_brute_force_and_lloyd(seed):
    rng = np.random.default_rng(seed)
    for k in (1, 2, 3, 4):
        n = int(rng.integers(k + 2, 30 if k > 2 else 400))
        if seed % 3 == 0:
            x = rng.integers(0, 12, size=n).astype(np.float64) / 7          # many repeated values
        elif seed % 3 == 1:
            x = np.concatenate([rng.normal(m, 0.3, size=n // 3 + 1) for m in (0, 2, 5)])[:n]
        else:
            x = rng.exponential(1e-3, size=n) + 1e6 * (seed == 5)             # large offset, small spread
        if len(np.unique(x)) < k:
            continue
        lab, cut = kmeans_1d(x, k)
        groups = [np.flatnonzero(lab == q) for q in range(1, k + 1)]
        cost = _sse(x, groups)
        best, parts, u = _brute(x, k) if len(np.unique(x)) <= 40 or k <= 2 else (None, None, None)
        if best is not None:
            assert abs(cost - best) <= 1e-12 * max(best, 1e-300) + 1e-18, (seed, k, cost, best)
            if len(parts) == 1:
                b = parts[0]
                want = [np.flatnonzero((x >= u[b[q]]) & (x <= u[b[q + 1] - 1])) for q in range(k)]
                got = sorted((tuple(g) for g in groups), key=lambda t: x[list(t)].min())
                assert [tuple(w) for w in want] == got, (seed, k)
        lloyd_rng = np.random.default_rng(1000 + seed)
        assert cost <= min(_lloyd(x, k, lloyd_rng) for _ in range(200)) * (1 + 1e-12) + 1e-18
        # relabel: label 1 is the largest cluster, sizes descend, equal sizes by ascending mean; cutoff = max of label 1
        sizes = [len(g) for g in groups]
        assert all(sizes[q] >= sizes[q + 1] for q in range(k - 1)) and min(sizes) > 0
        for q in range(k - 1):
            if sizes[q] == sizes[q + 1]:
                assert x[groups[q]].mean() < x[groups[q + 1]].mean()
        assert cut == x[lab == 1].max()
        # clusters are contiguous in sorted order and equal values share one
        for q in range(k):
            lo, hi = x[groups[q]].min(), x[groups[q]].max()
            assert np.all(lab[(x >= lo) & (x <= hi)] == q + 1)
        lab2, cut2 = kmeans_1d(x.copy(), k)
        assert np.array_equal(lab, lab2) and cut == cut2


def test_kmeans_ties_and_errors():
    # two equally good partitions of {0, 1, 2} into 2: ties go to the smallest split point ({0} | {1, 2})
    lab, cut = kmeans_1d([0.0, 1.0, 2.0], 2)
    assert lab.tolist() == [2, 1, 1] and cut == 2.0
    # equal sizes: ascending mean first
    lab, cut = kmeans_1d([10.0, 10.0, 0.0, 0.0], 2)
    assert lab.tolist() == [2, 2, 1, 1] and cut == 0.0
    lab, cut = kmeans_1d([3.0, 3.0, 3.0], 1)
    assert lab.tolist() == [1, 1, 1] and cut == 3.0
    with pytest.raises(ValueError, match="more cluster centers than distinct data points."):
        kmeans_1d([1.0, 1.0, 2.0], 3)
    with pytest.raises(ValueError, match="more cluster centers than distinct data points."):
        kmeans_1d(np.zeros(0), 1)
    with pytest.raises(ValueError):
        kmeans_1d([1.0, np.nan, 2.0], 2)
    with pytest.raises(ValueError):
        kmeans_1d([1.0, 2.0], 0)


def test_kmeans_up_to_255_clusters():
    rng = np.random.default_rng(3)
    x = rng.random(3000)
    for k in (8, 255):
        lab, cut = kmeans_1d(x, k)
        assert sorted(set(lab.tolist())) == list(range(1, k + 1))
        assert cut == x[lab == 1].max()


# ---------------------------------------------------------------------------------------------------------------------------------------
# GFF3 / reference FASTA readers
# ---------------------------------------------------------------------------------------------------------------------------------------
GFF = ("##gff-version 3\n"
       "# a comment\n"
       "\n"
       "chr\tsrc\tgene\t1\t30\t.\t+\t.\tID=g1\n"
       "chr\tsrc\tCDS\t2\t28\t.\t+\t0\tID=c1\n"
       "other\tsrc\tcds\t40\t55\t.\t-\t0\tID=c2\n"
       "chr\tsrc\tCds\t57\t60\t.\t-\t0\tID=c3\n"
       "##FASTA\n"
       ">chr\nACGT\n")
REF = ">chr1 some description\nACGTacgtNN\nRYKM-ACGTA\r\nCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCCC\n>second\nTTTT\n"


def _write(path, text, eol="\n", gz=False):
    data = text.replace("\r\n", "\n").replace("\n", eol).encode()
    if gz:
        with gzip.open(path, "wb") as fh:
            fh.write(data)
    else:
        path.write_bytes(data)
    return str(path)


@pytest.mark.parametrize("eol,gz", [("\n", False), ("\r\n", False), ("\n", True)])
def test_parse_gff_file(tmp_path, eol, gz):
    gp = _write(tmp_path / ("a.gff3.gz" if gz else "a.gff3"), GFF, eol, gz)
    rp = _write(tmp_path / ("r.fa.gz" if gz else "r.fa"), REF, eol, gz)
    ann = cds.parse_gff_file(gp, rp)
    assert ann.ref_name == "chr1" and ann.g == 60
    assert bytes(ann.ref[:20]) == b"ACGTacgtNNRYKM-ACGTA" and ann.ref.dtype == np.uint8      # lower case kept, first record only
    assert ann.gff["type"].tolist() == ["gene", "CDS", "cds", "Cds"]                          # stops at ##FASTA
    assert ann.gff["start"].tolist() == [1, 2, 40, 57] and ann.gff["end"].tolist() == [30, 28, 55, 60]
    assert ann.gff["seqid"].tolist() == ["chr", "chr", "other", "chr"]


def test_parse_gff_file_errors(tmp_path):
    rp = _write(tmp_path / "r.fa", REF)
    bad = _write(tmp_path / "bad.gff3", "##gff-version 3\nchr\tsrc\tCDS\t2\t28\t.\t+\n")
    with pytest.raises(ValueError, match="line 2"):
        cds.parse_gff_file(bad, rp)
    for body, msg in (("chr\ts\tCDS\t-1\t5\t.\t+\t0\tx\n", "Invalid start position found!"),
                      ("chr\ts\tCDS\t5\t61\t.\t+\t0\tx\n", "Invalid stop position found!"),
                      ("chr\ts\tCDS\t9\t5\t.\t+\t0\tx\n", "Invalid start-stop pair found!")):
        p = _write(tmp_path / "e.gff3", body)
        with pytest.raises(ValueError, match=msg):
            cds.parse_gff_file(p, rp)
        ann = cds.parse_gff_file(p, rp, perform_length_check=False)
        assert len(ann.gff) == 1
    with pytest.raises(ValueError, match="empty sequence!"):
        cds.parse_gff_file(_write(tmp_path / "ok.gff3", GFF), _write(tmp_path / "empty.fa", ">x\n"))
    with pytest.raises(FileNotFoundError):
        cds.parse_gff_file(str(tmp_path / "missing.gff3"), rp)


def test_annotation_from_arrays_and_arguments():
    ann = cds.Annotation.from_arrays([1, 10], [5, 20], "ACGTACGTACGTACGTACGTAC")
    assert ann.g == 22 and ann.gff["type"].tolist() == ["CDS", "CDS"] and ann.ref.dtype == np.uint8
    with pytest.raises(ValueError, match="Provide either one of gbk or gff"):
        cds.estimate_variation_in_CDS(None)
    with pytest.raises(ValueError, match="Provide either one of gbk or gff"):
        cds.estimate_variation_in_CDS(None, gbk=object(), gff=ann)
    with pytest.raises(NotImplementedError):
        cds.estimate_variation_in_CDS(None, gbk=object())


def test_cdsvar_old_style_construction():
    cv = CdsVar(paint=np.array([1, 2, 3]), nclust=3)
    assert cv.nclust == 3 and cv.paint.tolist() == [1, 2, 3]
    assert cv.var_estimate is None and cv.clusts is None and cv.allele_table is None and cv.alt is None and cv.ref is None
    import ldweaver_amd
    assert ldweaver_amd.CdsVar is CdsVar and ldweaver_amd.estimate_variation_in_CDS is cds.estimate_variation_in_CDS
    assert ldweaver_amd.kmeans_1d is kmeans_1d and ldweaver_amd.parse_gff_file is cds.parse_gff_file
