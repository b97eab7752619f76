"""The device short-range model — ldw_sr_excess_stats[_blocks], ldw_sr_pvalues (k_sr_dstar, k_sr_pval, k_sr_pool) and the host
steps of srp.merge_n_sort_sr_links_device — against mergeNsort_sr_links (R/computePairwiseMI.R:400-495) at its edges: lens at 0, 1, S,
S + 1 and g / 2, the positional mean_dist[len] lookup (Q5), excesses of exactly 0, rows either side of the cut-off's crossing and of the
continued fraction's branch point, cross-cluster rows with tied p-values and with one key held by two table rows, the pool's MI tie,
empty and one-row tables, tables past the grid-stride limits and the 2^22-row floor, and 1..255 clusters.

Every table is placed with ``Engine.links_import`` (no MI pass); the alignment only satisfies set_alignment / set_snp_meta.  Stage cases
use a hand-chosen mean_dist and beta shape and ``np_sr_reduce``, a vectorised restatement of R/computePairwiseMI.R:444-490 that a CPU
test of this file checks against the oracle's literal one; end-to-end cases run the whole model against the oracle."""
import os

import mpmath
import numpy as np
import pytest
from scipy import special

import ldw_oracle as orc
from ldweaver_amd import srp as SRP
from ldweaver_amd.synth import synth_alignment

G = 50_000_000
E32 = np.zeros(0, dtype=np.int32)
E64 = np.zeros(0, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------------------------
def ref_srp(x, a: float, b: float) -> np.ndarray:
    """-pbeta(x, a, b, lower.tail = FALSE, log.p = TRUE) to ~1e-14 relative: -log1p(-I_x(a, b)) below the mean, where the lower tail is
    the small one, -log(I_{1-x}(b, a)) above it, mpmath where that underflows (orc.neg_log_beta_sf)."""
    x = np.asarray(x, dtype=np.float64)
    low = x < a / (a + b)
    out = np.empty(x.shape)
    out[low] = -np.log1p(-special.betainc(a, b, x[low]))
    with np.errstate(divide="ignore"):
        out[~low] = -np.log(special.betaincc(a, b, x[~low]))
    deep = ~low & (~np.isfinite(out) | (out > 600.0)) & (x < 1.0)
    if deep.any():
        out[deep] = orc.neg_log_beta_sf(x[deep], a, b)
    return out


def mp_srp(x: float, a: float, b: float) -> float:
    """The same tail in 50-digit arithmetic."""
    with mpmath.workdps(50):
        return float(-mpmath.log(mpmath.betainc(a, b, mpmath.mpf(x), 1, regularized=True)))


def mp_crossing(a: float, b: float, cutoff: float) -> float:
    """The excess x* with -log P(X > x*) == cutoff (bisection in log x, 50 digits)."""
    with mpmath.workdps(50):
        f = lambda lx: -mpmath.log(mpmath.betainc(a, b, mpmath.exp(lx), 1, regularized=True)) - cutoff
        lo, hi = mpmath.mpf(-800), mpmath.mpf(-1e-30)
        for _ in range(400):
            mid = (lo + hi) / 2
            if f(mid) > 0:
                hi = mid
            else:
                lo = mid
        return float(mpmath.exp(hi))


def _shape3(shape):
    """(nclust, 3) rows a, b, log B(a, b) as ldw_sr_pvalues takes them."""
    s = np.asarray(shape, dtype=np.float64)
    return np.column_stack([s[:, 0], s[:, 1], [SRP._betaln(float(p), float(q)) for p, q in s[:, :2]]])


def np_sr_reduce(a, b, mi, POS, paint, g, sr_dist, md, shape, cutoff, srp=ref_srp, keep_srp=None):
    """R/computePairwiseMI.R:444-490 on the table (a, b, mi) — a = from side (pos2), b = to side (pos1) — given mean_dist per cluster
    ``md`` (nclust, S), NaN past its length, and the beta shapes ``shape`` (nclust, >= 2).

    Cluster i's table holds the rows touching cluster i in table order; rows with len in (0, sr_dist) whose excess MI - mean_dist[len]
    (Q5: indexed by the value of len, NA past the table, :448) is > 0 get srp = srp(excess) (:453).  Rows inside one cluster are kept
    as they are; the copies of a cross-cluster row (clust1 != clust2) are grouped by (pos1, pos2, clust1, clust2, len, MI), groups in
    order of first appearance in the clusters' concatenation, and the first copy of largest srp stands for the group (:478-485).  The
    merged table is cut at srp > cutoff (:488) — judged on ``keep_srp[row]`` when given (a device's own p-values) — and the ARACNE
    check set is its rows with MI >= min(MI kept) (:489).

    Returns (red, chk): dicts of table row, clust_c, first_clust (the cluster of first appearance), dup, srp_max, in the reference's
    row order."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    mi = np.asarray(mi, dtype=np.float64)
    POS, paint = np.asarray(POS, dtype=np.float64), np.asarray(paint, dtype=np.int64)
    md, shape = np.asarray(md, dtype=np.float64), np.asarray(shape, dtype=np.float64)
    nclust, S = md.shape
    n = len(mi)
    ln = orc.circ_len(POS[b], POS[a], g) if n else E64
    valid = (ln < sr_dist) & (ln > 0)
    li = np.where(valid, ln, 0).astype(np.int64)
    c1, c2 = paint[b], paint[a]

    def excess(c):
        ok = valid & (li <= S)
        e = np.full(n, np.nan)
        e[ok] = mi[ok] - md[c[ok] - 1, li[ok] - 1]
        return e

    e1, e2 = excess(c1), excess(c2)
    v1, v2 = e1 > 0, (c1 != c2) & (e2 > 0)
    s1, s2 = np.full(n, np.nan), np.full(n, np.nan)
    for c in np.unique(np.r_[c1[v1], c2[v2]]):
        for v, e, cl, s in ((v1, e1, c1, s1), (v2, e2, c2, s2)):
            m = v & (cl == c)
            if m.any():
                s[m] = srp(e[m], float(shape[c - 1, 0]), float(shape[c - 1, 1]))
    row = np.arange(n)
    dupr = c1 != c2
    # the rows inside one cluster, per cluster in table order
    mrow = row[v1 & ~dupr]
    mrow = mrow[np.lexsort((mrow, c1[mrow]))]
    # the copies of the cross-cluster rows in the order of the clusters' concatenation (cluster, then table row)
    crow = np.r_[row[v1 & dupr], row[v2]]
    ccl = np.r_[c1[v1 & dupr], c2[v2]]
    csrp = np.r_[s1[v1 & dupr], s2[v2]]
    o = np.lexsort((crow, ccl))
    crow, ccl, csrp = crow[o], ccl[o], csrp[o]
    if len(crow):
        key = np.column_stack([POS[b[crow]], POS[a[crow]], c1[crow], c2[crow], ln[crow], mi[crow]])
        _, first, grp = np.unique(key, axis=0, return_index=True, return_inverse=True)
        grp = grp.reshape(-1)
        rank = np.argsort(np.argsort(first, kind="stable"), kind="stable")     # groups in order of first appearance
        gi = rank[grp]
        pick = np.lexsort((np.arange(len(crow)), -csrp, gi))                      # per group: largest srp, then the first copy
        head = np.ones(len(pick), dtype=bool)
        head[1:] = gi[pick][1:] != gi[pick][:-1]
        win = pick[head]
        drow, dcl, dsrp = crow[win], ccl[win], csrp[win]
        dfirst = ccl[np.sort(first)]
    else:
        drow = dcl = dfirst = np.zeros(0, dtype=np.int64)
        dsrp = E64
    tab = dict(row=np.r_[mrow, drow], clust_c=np.r_[c1[mrow], dcl], first_clust=np.r_[c1[mrow], dfirst],
               dup=np.r_[np.zeros(len(mrow), dtype=bool), np.ones(len(drow), dtype=bool)], srp_max=np.r_[s1[mrow], dsrp])
    judged = tab["srp_max"] if keep_srp is None else np.asarray(keep_srp)[tab["row"]]
    kept = judged > cutoff
    red = {k: v[kept] for k, v in tab.items()}
    in_chk = mi[tab["row"]] >= mi[red["row"]].min() if kept.any() else np.zeros(len(kept), dtype=bool)
    return red, {k: v[in_chk] for k, v in tab.items()}


def _by_clust(tab, nclust):
    return [{k: v[(tab["clust1"] == ci) | (tab["clust2"] == ci)] for k, v in tab.items()} for ci in range(1, nclust + 1)]


def _oracle_table(a, b, mi, POS, paint, g):
    POS = np.asarray(POS, dtype=np.float64)
    return dict(pos1=POS[b], pos2=POS[a], clust1=np.asarray(paint)[b], clust2=np.asarray(paint)[a], len=orc.circ_len(POS[b], POS[a], g),
                MI=np.asarray(mi, dtype=np.float64))


def _as_oracle_rows(red, a, b, mi, POS, paint, g):
    """np_sr_reduce's rows in the oracle's columns."""
    r = red["row"]
    t = _oracle_table(a, b, mi, POS, paint, g)
    out = {k: v[r] for k, v in t.items()}
    out["clust_c"], out["srp_max"] = red["clust_c"], red["srp_max"]
    return out


def _decay_table(rng, POS, paint, n, sr_dist, g, w=20):
    """Up to n short-range rows between SNPs at most w indices apart, each SNP pair once (as the pass writes them), either orientation,
    with an MI decaying in len on a 1/1024 grid (ties, shared keys)."""
    L = len(POS)
    a = rng.integers(0, L, 2 * n)
    b = a + rng.integers(1, w + 1, 2 * n)
    ok = b < L
    a, b = a[ok], b[ok]
    _, first = np.unique(a * L + b, return_index=True)
    first = np.sort(first)
    a, b = a[first], b[first]
    sw = rng.random(len(a)) < 0.5
    a, b = np.where(sw, b, a), np.where(sw, a, b)
    ln = orc.circ_len(POS[b].astype(float), POS[a].astype(float), g)
    ok = ln < sr_dist
    a, b, ln = a[ok][:n], b[ok][:n], ln[ok][:n]
    mi = 0.08 * (ln + 1) ** -0.25 + rng.exponential(0.03, len(a))
    return a.astype(np.int32), b.astype(np.int32), np.round(mi * 1024) / 1024


def _plant_triangles(rng, POS, a, b, mi, k):
    """k triangles (i, i + 1, i + 2) of SNPs at three distinct positions replace whatever rows those pairs had: MI 0.5 on the outer link,
    0.625 on the two inner ones, so that ARACNE finds the outer link indirect (R/io_functions.R:101-164)."""
    L = len(POS)
    ok = np.nonzero((POS[1:-1] > POS[:-2]) & (POS[2:] > POS[1:-1]))[0]
    ok = ok[ok % 5 == 0]
    tri = rng.choice(ok, min(k, len(ok)), replace=False)
    members = np.zeros(L, dtype=bool)
    members[np.r_[tri, tri + 1, tri + 2]] = True
    keep = ~(members[a] & members[b] & (np.abs(a.astype(np.int64) - b) <= 2))
    ta = np.r_[tri, tri, tri + 1]
    tb = np.r_[tri + 2, tri + 1, tri + 2]
    return (np.r_[a[keep], ta].astype(np.int32), np.r_[b[keep], tb].astype(np.int32),
            np.r_[mi[keep], np.full(len(tri), 0.5), np.full(2 * len(tri), 0.625)])


def _twin_positions(rng, L, step=7):
    """Positions of L SNPs where about a third of the positions are held by two SNPs (adjacent indices)."""
    u = np.cumsum(rng.integers(1, step, L))
    twin = rng.random(L) < 0.35
    twin[0] = False
    return np.where(twin, np.r_[u[0], u[:-1]], u)


def _twin_rows(POS, paint, a, b, mi):
    """For every row whose SNPs have a twin (another SNP at the same position with the same cluster), a copy of the row through the twin:
    the same key (pos1, pos2, clust1, clust2, len, MI) held by two table rows."""
    POS, paint = np.asarray(POS), np.asarray(paint)
    twin = np.full(len(POS), -1)
    for i in range(1, len(POS)):
        if POS[i] == POS[i - 1] and paint[i] == paint[i - 1]:
            twin[i - 1], twin[i] = i, i - 1
    sel = twin[a] >= 0
    return np.r_[a, twin[a[sel]]].astype(np.int32), np.r_[b, b[sel]].astype(np.int32), np.r_[mi, mi[sel]]


# ------------------------------------------------------------------------------------------------------------------------------
# CPU: np_sr_reduce against the oracle's literal mergeNsort_sr_links
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["three_clusters", "twins", "cross_only_ties", "fractional_sr_dist"])
def test_np_sr_reduce_equals_oracle(case):
    rng = np.random.default_rng(["three_clusters", "twins", "cross_only_ties", "fractional_sr_dist"].index(case) + 40)
    L, g = 160, 10_000.0
    sr_dist = 180.5 if case == "fractional_sr_dist" else 200.0
    nclust = 2 if case == "cross_only_ties" else 3
    POS = _twin_positions(rng, L) if case == "twins" else np.sort(rng.choice(np.arange(1, 1500), L, replace=False))
    paint = rng.integers(1, nclust + 1, L)
    if case == "twins":
        paint[1:][POS[1:] == POS[:-1]] = paint[:-1][POS[1:] == POS[:-1]]
    if case == "cross_only_ties":
        paint = 1 + np.arange(L) % 2
    a, b, mi = _decay_table(rng, POS, paint, 2500, sr_dist, g)
    if case == "cross_only_ties":       # every row joins clusters 1 and 2: both clusters see the same table, fit and p-values (exact ties)
        ok = paint[a] != paint[b]
        a, b, mi = a[ok], b[ok], mi[ok]
    if case == "twins":
        a, b, mi = _twin_rows(POS, paint, a, b, mi)
    tab = _oracle_table(a, b, mi, POS, paint, g)
    fit, shapes = [], []
    probe, _ = orc.merge_n_sort_sr_links(_by_clust(tab, nclust), nclust, sr_dist, -1e300, fit_data=fit, shapes=shapes)
    S = int(np.ceil(sr_dist)) - 1
    md = np.full((nclust, S), np.nan)
    for ci, f in enumerate(fit):
        md[ci, :len(f["fit"])] = f["fit"]                              # positional (Q5)
    cut = float(np.quantile(probe["srp_max"], 0.7))
    for cutoff in (-1e300, cut, float(probe["srp_max"].max())):
        ored, ochk = orc.merge_n_sort_sr_links(_by_clust(tab, nclust), nclust, sr_dist, cutoff)
        red, chk = np_sr_reduce(a, b, mi, POS, paint, g, sr_dist, md, np.array(shapes), cutoff, srp=orc.neg_log_beta_sf)
        for got, want in ((red, ored), (chk, ochk)):
            got = _as_oracle_rows(got, a, b, mi, POS, paint, g)
            for k in ("clust_c", "pos1", "pos2", "clust1", "clust2", "len", "MI", "srp_max"):
                assert np.array_equal(np.asarray(got[k], dtype=float), np.asarray(want[k], dtype=float)), (case, cutoff, k)
    assert len(probe["MI"]) > 100 and (probe["clust1"] != probe["clust2"]).any()
    if case == "cross_only_ties":
        assert np.array_equal(md[0], md[1], equal_nan=True) and shapes[0] == shapes[1] and (probe["clust_c"] == 1).all()
    if case == "twins":             # the oracle merged the rows that share a key: fewer rows than the table's positive excesses
        red, _ = np_sr_reduce(a, b, mi, POS, paint, g, sr_dist, md, np.array(shapes), -1e300, srp=orc.neg_log_beta_sf)
        assert len(red["row"]) == len(probe["MI"])
        assert len(np.unique(np.column_stack([tab["pos1"], tab["pos2"], tab["MI"]])[red["row"][red["dup"]]], axis=0)) == red["dup"].sum()


# ------------------------------------------------------------------------------------------------------------------------------
# GPU: helpers
# ------------------------------------------------------------------------------------------------------------------------------
_ALN = {}


def _place(engine, POS, paint, a, b, mi, g=G):
    """Alignment of len(POS) SNPs, the given positions / clusters, and (a, b, mi) as the short-range table."""
    L = len(POS)
    if L not in _ALN:
        st = np.ascontiguousarray(synth_alignment(L, 16, seed=L)["states"])
        _ALN[L] = (st, *orc.uqe_r(st))
    st, uqe, r = _ALN[L]
    engine.set_alignment(st)
    engine.set_snp_meta(r, uqe, np.asarray(POS, dtype=np.int32), np.asarray(paint, dtype=np.int32), float(g))
    engine.links_import(0, np.asarray(a, dtype=np.int32), np.asarray(b, dtype=np.int32), np.asarray(mi, dtype=np.float64))
    engine.links_import(1, E32, E32, E64)


def _ref_order(red):
    """The reference's row order of the device's reduced rows (srp.merge_n_sort_sr_links_device): rows inside one cluster per cluster,
    then the cross-cluster rows by the cluster of first appearance; table order within both."""
    key_cl = np.where(red["dup"], red["first_clust"], red["clust_c"])
    return np.lexsort((red["row"], key_cl, red["dup"]))


def _device(engine, nclust, sr_dist, md, shape, cutoff, pval_all=False):
    engine.sr_len_quantiles(nclust, sr_dist, 0.95)
    if pval_all:
        os.environ["LDW_SR_PVAL_ALL"] = "1"
    try:
        n_red, n_pool, mn = engine.sr_pvalues(md, _shape3(shape), cutoff)
    finally:
        os.environ.pop("LDW_SR_PVAL_ALL", None)
    red = engine.sr_reduced()
    red = {k: v[_ref_order(red)] for k, v in red.items()}
    return n_red, n_pool, mn, red, engine.sr_pool()


def _stage_case(engine, POS, paint, a, b, mi, sr_dist, md, shape, cutoff, g=G, check_all=True):
    """Device p-values, cut and pool on the placed table against np_sr_reduce with the hand-chosen md / shape: the kept set judged by the
    reference's rule on the device's own srp_max (from a run with cut-off -1), srp_max against ref_srp to 2e-10, identical cluster columns,
    the pool equal to the check set.  check_all: the early skip of k_sr_dstar against LDW_SR_PVAL_ALL=1 too.  Returns (red, all)."""
    a, b, mi = np.asarray(a, dtype=np.int32), np.asarray(b, dtype=np.int32), np.asarray(mi, dtype=np.float64)
    POS, paint = np.asarray(POS), np.asarray(paint)
    nclust = md.shape[0]
    _place(engine, POS, paint, a, b, mi, g)
    # every positive excess, with its srp_max
    n_all, n_pool_all, mn_all, dall, _ = _device(engine, nclust, sr_dist, md, shape, -1.0)
    want_all, _ = np_sr_reduce(a, b, mi, POS, paint, g, sr_dist, md, shape, -1.0)
    keep = SRP.merged_key_rows(POS, paint, a[dall["row"]], b[dall["row"]], mi[dall["row"]], dall["dup"])
    dall = {k: v[keep] for k, v in dall.items()}
    for k in ("row", "clust_c", "first_clust", "dup"):
        assert np.array_equal(dall[k], want_all[k]), k
    np.testing.assert_allclose(dall["srp_max"], want_all["srp_max"], rtol=2e-10, atol=1e-13)
    assert n_all == n_pool_all >= len(want_all["row"])
    dev_srp = np.full(len(mi), np.nan)
    dev_srp[dall["row"]] = dall["srp_max"]
    # the cut and the pool
    n_red, n_pool, mn, red, pool = _device(engine, nclust, sr_dist, md, shape, cutoff)
    want, chk = np_sr_reduce(a, b, mi, POS, paint, g, sr_dist, md, shape, cutoff, keep_srp=dev_srp)
    keep = SRP.merged_key_rows(POS, paint, a[red["row"]], b[red["row"]], mi[red["row"]], red["dup"])
    assert n_red == len(red["row"])
    red = {k: v[keep] for k, v in red.items()}
    for k in ("row", "clust_c", "first_clust", "dup"):
        assert np.array_equal(red[k], want[k]), k
    assert np.array_equal(red["srp_max"], dev_srp[want["row"]])      # (the same kernel on the same row, bit for bit)
    assert np.array_equal(red["MI"], mi[red["row"]]) and np.array_equal(red["a"], a[red["row"]]) and np.array_equal(red["b"], b[red["row"]])
    if len(want["row"]) == 0:
        assert n_red == n_pool == 0 and np.isnan(mn) and len(pool[0]) == 0 and len(engine.aracne_device()) == 0
    else:
        assert mn == mi[want["row"]].min()
        pa, pb, pm = pool
        pkeep = SRP.merged_key_rows(POS, paint, pa, pb, pm, paint[pa] != paint[pb])
        got = np.sort(np.rec.fromarrays([pa[pkeep], pb[pkeep], pm[pkeep]]))
        # (of two pool rows that share a key either may stand for it: compare the key, not the SNP)
        wr = chk["row"]
        wkey = np.sort(np.rec.fromarrays([POS[a[wr]], POS[b[wr]], mi[wr]]))
        assert np.array_equal(np.sort(np.rec.fromarrays([POS[got.f0], POS[got.f1], got.f2])), wkey)
    if check_all:
        n0, np0, mn0, red0, _ = _device(engine, nclust, sr_dist, md, shape, cutoff, pval_all=True)
        assert (n0, np0) == (n_red, n_pool) and (mn0 == mn or (np.isnan(mn0) and np.isnan(mn)))
        keep0 = SRP.merged_key_rows(POS, paint, a[red0["row"]], b[red0["row"]], mi[red0["row"]], red0["dup"])
        for k in ("row", "clust_c", "first_clust", "dup", "srp_max"):
            assert np.array_equal(red0[k][keep0], red[k]), k
    return red, dall


def _md(nclust, S, k, level=2.0 ** -6):
    """A decay of k entries (cluster c: level * (1 + ((c - 1) mod 4) / 4) * len^-0.25), NaN past them (Q5)."""
    md = np.full((nclust, S), np.nan)
    md[:, :k] = level * (1.0 + 0.25 * (np.arange(nclust)[:, None] % 4)) * np.arange(1, k + 1, dtype=np.float64)[None, :] ** -0.25
    return md


SH3 = np.array([[0.4, 60.0], [2.5, 40.0], [0.5, 500.0]])   # (tails of the tables' excesses stay within what mpmath resolves)


# ------------------------------------------------------------------------------------------------------------------------------
# GPU: lengths, Q5, exact zeros
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sr_dist", [500.0, 500.5, 65535.0])
def test_lengths_at_their_edges(engine, sr_dist):
    """len 1, S - 1, S, S + 1 (S = ceil(sr_dist) - 1: len < sr_dist is strict), lens across the origin of the circular genome and
    repeated positions (len 0), every row with a positive excess in the cluster it touches."""
    S = int(np.ceil(sr_dist)) - 1
    g = 1_000_000
    anchors = [100, 200_000, 400_000]
    POS, rows = [], []
    for p in anchors:
        base = len(POS)
        offs = [0, 1, S - 1, S, S + 1, S + 2, 0]                        # the last: a second SNP at the anchor's position
        POS += [p + o for o in offs]
        rows += [(base, base + j) for j in range(1, len(offs))]
    base = len(POS)                                                      # across the origin: g - 3 .. g + 2 (mod g)
    POS += [g - 3, g - 1, 2, 5, S - 4]
    rows += [(base, base + 1), (base, base + 2), (base + 1, base + 3), (base, base + 4), (base + 1, base + 4)]
    POS = np.asarray(POS)
    order = np.argsort(POS, kind="stable")
    inv = np.empty_like(order)
    inv[order] = np.arange(len(order))
    POS = POS[order]
    rows = np.array(rows)
    L = len(POS)
    paint = np.ones(L, dtype=np.int32)
    a, b = inv[rows[:, 0]], inv[rows[:, 1]]
    a, b = np.r_[a, b], np.r_[b, a]                                      # both orientations (pos1 / pos2 swapped)
    mi = np.linspace(0.2, 0.6, len(a))
    md = np.full((1, S), 0.1)
    red, _ = _stage_case(engine, POS, paint, a, b, mi, sr_dist, md, SH3[:1], 2.0, g=g)
    ln = orc.circ_len(POS[b].astype(float), POS[a].astype(float), float(g))
    _, dall = _stage_case(engine, POS, paint, a, b, mi, sr_dist, md, SH3[:1], -1.0, g=g, check_all=False)
    lens = set(ln[dall["row"]].astype(int).tolist())
    assert {1, S - 1, S} <= lens and S + 1 not in lens and 0 not in lens and max(lens) == S
    assert (ln == 0).sum() >= 6 and (ln == S + 1).sum() >= 6


@pytest.mark.gpu
def test_half_genome_length(engine):
    """A small even genome with sr_dist > g / 2: len = g / 2 is the longest length there is."""
    g, sr_dist = 40, 30.0
    POS = np.arange(1, 41)
    L = len(POS)
    a, b = np.triu_indices(L, 1)
    paint = 1 + (np.arange(L) % 2)
    rng = np.random.default_rng(1)
    mi = np.round(rng.uniform(0.05, 0.5, len(a)) * 256) / 256
    md = _md(2, 29, 29, level=0.1)
    _stage_case(engine, POS, paint, a, b, mi, sr_dist, md, SH3[:2], 1.5, g=g)
    ln = orc.circ_len(POS[b].astype(float), POS[a].astype(float), float(g))
    assert ln.max() == 20 and (ln == 20).sum() == 20


@pytest.mark.gpu
def test_q5_lookup_past_the_fitted_lengths(engine):
    """Cluster 1's mean_dist has k = 7 entries, cluster 2's 300: rows at len k, k + 1 and far beyond read NA in cluster 1 and leave its
    statistics, p-values and pool; cross-cluster rows there take cluster 2's value alone (first_clust = clust_c = 2)."""
    k, sr_dist = 7, 500.0
    S = 499
    rng = np.random.default_rng(2)
    POS = np.r_[np.arange(0, 40) + 1000, np.arange(0, 40) * 11 + 2000]
    L = len(POS)
    paint = np.r_[np.ones(20), 2 * np.ones(20), np.ones(20), 2 * np.ones(20)].astype(np.int32)[rng.permutation(L)]
    a, b = np.triu_indices(L, 1)
    ln = orc.circ_len(POS[b].astype(float), POS[a].astype(float), float(G))
    ok = ln < sr_dist
    a, b = a[ok], b[ok]
    mi = np.round(rng.uniform(0.01, 0.3, len(a)) * 1024) / 1024
    md = np.full((2, S), np.nan)
    md[0, :k] = 0.05
    md[1, :300] = 0.08
    red, dall = _stage_case(engine, POS, paint, a, b, mi, sr_dist, md, SH3[:2], 0.5)
    ln = orc.circ_len(POS[b].astype(float), POS[a].astype(float), float(G))
    lk = ln[dall["row"]]
    c1_rows = dall["clust_c"] == 1
    assert lk[c1_rows].max() == k and (lk[~c1_rows] > k).any() and (lk > 300).sum() == 0
    cross_past = dall["dup"] & (lk > k)
    assert cross_past.sum() > 10 and (dall["first_clust"][cross_past] == 2).all()
    # the excess statistics read the same lookup
    stats = engine.sr_excess_stats(md)
    _stats_match(stats, a, b, mi, POS, paint, G, sr_dist, md)


@pytest.mark.gpu
def test_excess_exactly_zero_and_one_ulp(engine):
    """MI == mean_dist bitwise (excess 0: not > 0, out of the statistics, p-values and pool) and one ulp either side."""
    POS = np.arange(1, 31) * 10
    L = len(POS)
    paint = np.ones(L, dtype=np.int32)
    paint[15:] = 2
    a, b = np.triu_indices(L, 1)
    ln = orc.circ_len(POS[b].astype(float), POS[a].astype(float), float(G))
    ok = ln < 200
    a, b, ln = a[ok], b[ok], ln[ok]
    md = _md(2, 199, 199, level=0.1)
    c1 = paint[b]
    base = md[c1 - 1, ln.astype(int) - 1]
    which = np.arange(len(a)) % 4
    mi = np.where(which == 0, base, np.where(which == 1, np.nextafter(base, 1), np.where(which == 2, np.nextafter(base, 0), base + 0.05)))
    _, dall = _stage_case(engine, POS, paint, a, b, mi, 200.0, md, SH3[:2], 1e-12)
    w = which[dall["row"]]
    same = paint[a[dall["row"]]] == paint[b[dall["row"]]]
    assert (w[same] == 0).sum() == 0 and (w[same] == 2).sum() == 0 and (w[same] == 1).sum() > 10
    stats = engine.sr_excess_stats(md)
    _stats_match(stats, a, b, mi, POS, paint, G, 200.0, md)


# ------------------------------------------------------------------------------------------------------------------------------
# GPU: the cut-off and its crossing
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cutoff_equal_to_a_rows_srp(engine):
    """srp > cutoff is strict: a cut-off equal to the device's own srp_max of a row drops that row and keeps the next larger one."""
    rng = np.random.default_rng(3)
    POS = np.arange(1, 61) * 5
    L = len(POS)
    paint = rng.integers(1, 4, L).astype(np.int32)
    a, b = np.triu_indices(L, 1)
    mi = np.round(rng.uniform(0.02, 0.4, len(a)) * 4096) / 4096
    md = _md(3, 299, 299)
    _place(engine, POS, paint, a, b, mi)
    _, _, _, dall, _ = _device(engine, 3, 300.0, md, SH3, -1.0)
    s = np.unique(dall["srp_max"])
    for q in (0.2, 0.5, 0.9, 0.999):
        cut = float(s[int(q * (len(s) - 1))])
        red, _ = _stage_case(engine, POS, paint, a, b, mi, 300.0, md, SH3, cut, check_all=q == 0.5)
        assert red["srp_max"].min() == s[s > cut].min() and (dall["srp_max"] == cut).sum() >= 1
        assert len(red["row"]) == (dall["srp_max"] > cut).sum()


@pytest.mark.gpu
@pytest.mark.parametrize("sh,cutoff", [((0.4, 60.0), 3.0), ((2.5, 40.0), 3.0), ((2.5, 40.0), 0.05), ((0.5, 5.0e4), 6.0),
                                       ((1.0, 8.0), 1.5), ((0.3, 50.0), 1e-20)])
def test_rows_either_side_of_the_crossing(engine, sh, cutoff):
    """Rows at excesses x*(1 +- 1e-7), x*(1 +- 2e-6) around the mpmath crossing x* of the cut-off, at the continued fraction's branch
    point (a + 1) / (a + b + 2) and one ulp either side of it.  The last shape's crossing (~1e-68) lies below what k_sr_dstar's 200 halvings
    reach: its fallback (every positive excess evaluated) decides there."""
    a_, b_ = sh
    xs = mp_crossing(a_, b_, cutoff)
    bp = (a_ + 1.0) / (a_ + b_ + 2.0)
    ex = np.array([xs * (1 - 2e-6), xs * (1 - 1e-7), xs, xs * (1 + 1e-7), xs * (1 + 2e-6), xs * 2, xs * 0.5,
                   np.nextafter(bp, 0), bp, np.nextafter(bp, 1)])
    level = 2.0 ** -230 if xs < 1e-50 else 2.0 ** -12          # md + x must hold x to ~1e-14
    L = 2 * len(ex) + 2
    POS = np.arange(1, L + 1) * 3
    a = np.arange(0, L, 2)[:len(ex)]
    b = a + 1
    md = np.full((1, 99), level)
    mi = level + ex
    x = mi - level
    want = np.array([mp_srp(v, a_, b_) for v in x])
    red, dall = _stage_case(engine, POS, np.ones(L, dtype=np.int32), a, b, mi, 100.0, md, np.array([sh]), cutoff)
    got = np.full(len(ex), np.nan)
    got[dall["row"]] = dall["srp_max"]
    np.testing.assert_allclose(got, want, rtol=2e-10, atol=1e-300)
    kept = np.isin(np.arange(len(ex)), red["row"])
    assert kept[3] and kept[4] and not kept[0] and not kept[1]
    other = np.arange(len(ex)) != 2                          # (x* itself: within rounding of the cut-off)
    assert (kept == (want > cutoff))[other].all()


# ------------------------------------------------------------------------------------------------------------------------------
# GPU: cross-cluster rows
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cross_cluster_ties_and_one_sided_excess(engine):
    """Clusters 1 and 2 with the same mean_dist and shape: every cross-cluster row ties exactly and goes to cluster 1 whichever side holds it
    (which.max: the first copy, :484); cluster 3's decay lies above most MI values, so rows between 2 and 3 mostly have a positive excess in
    cluster 2 only (first_clust = clust_c = 2), and rows between 1 and 3 in cluster 1 only."""
    rng = np.random.default_rng(4)
    POS = np.arange(1, 91) * 4
    L = len(POS)
    paint = rng.integers(1, 4, L).astype(np.int32)
    a, b = np.triu_indices(L, 1)
    ln = orc.circ_len(POS[b].astype(float), POS[a].astype(float), float(G))
    ok = ln < 300
    a, b = a[ok], b[ok]
    mi = np.round(rng.uniform(0.01, 0.25, len(a)) * 2048) / 2048
    md = np.full((3, 299), np.nan)
    md[0] = md[1] = 0.06
    md[2] = 0.2
    shape = np.array([[0.6, 30.0], [0.6, 30.0], [1.5, 20.0]])
    red, dall = _stage_case(engine, POS, paint, a, b, mi, 300.0, md, shape, 0.3)
    c1, c2 = paint[b[dall["row"]]], paint[a[dall["row"]]]
    t12 = dall["dup"] & (np.minimum(c1, c2) == 1) & (np.maximum(c1, c2) == 2)
    assert t12.sum() > 50 and (dall["clust_c"][t12] == 1).all() and ((c1 == 2) & t12).sum() > 20
    t23 = dall["dup"] & (np.minimum(c1, c2) == 2) & (np.maximum(c1, c2) == 3)
    assert (dall["first_clust"][t23] == 2).sum() > 10
    t13 = dall["dup"] & (np.minimum(c1, c2) == 1) & (np.maximum(c1, c2) == 3)
    assert ((dall["first_clust"][t13] == 1) & (dall["clust_c"][t13] == 1)).sum() > 10


@pytest.mark.gpu
def test_cross_cluster_key_held_by_two_rows(engine):
    """Two SNPs at one position with the same cluster and the same MI towards a third SNP of another cluster: two table rows with one key
    (pos1, pos2, clust1, clust2, len, MI).  R's data.table groups them into ONE reduced row (:478-485); rows inside one cluster stay two."""
    rng = np.random.default_rng(5)
    L = 120
    POS = _twin_positions(rng, L)
    paint = rng.integers(1, 3, L).astype(np.int32)
    tw = np.r_[False, POS[1:] == POS[:-1]]
    paint[tw] = paint[np.nonzero(tw)[0] - 1]
    a, b, mi = _decay_table(rng, POS, paint, 3000, 400.0, float(G))
    a, b, mi = _twin_rows(POS, paint, a, b, mi)
    md = _md(2, 399, 399, level=0.05)
    red, dall = _stage_case(engine, POS, paint, a, b, mi, 400.0, md, SH3[:2], 1.0)
    kp = np.column_stack([POS[b[dall["row"]]], POS[a[dall["row"]]], mi[dall["row"]]])
    d = dall["dup"]
    assert len(np.unique(kp[d], axis=0)) == d.sum() > 50
    assert len(np.unique(kp[~d], axis=0)) < (~d).sum()       # inside one cluster both rows stay


@pytest.mark.gpu
def test_merge_n_sort_merges_rows_that_share_a_key(engine):
    """srp.merge_n_sort_sr_links_device on a table whose twins share keys: one row per cross-cluster key, as the oracle."""
    rng = np.random.default_rng(6)
    L, sr_dist = 150, 400.0
    POS = _twin_positions(rng, L)
    paint = rng.integers(1, 3, L).astype(np.int32)
    tw = np.r_[False, POS[1:] == POS[:-1]]
    paint[tw] = paint[np.nonzero(tw)[0] - 1]
    a, b, mi = _decay_table(rng, POS, paint, 6000, sr_dist, float(G))
    a, b, mi = _twin_rows(POS, paint, *_plant_triangles(rng, POS, a, b, mi, 15))
    _e2e_case(engine, POS, paint, a, b, mi, 2, sr_dist)


# ------------------------------------------------------------------------------------------------------------------------------
# GPU: pool and small tables
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pool_mi_tie_at_the_minimum_kept(engine):
    """Rows of cluster 2 whose MI equals min(MI kept) exactly but whose p-value does not pass are in the pool (>=, :489); rows one ulp
    below it, with a positive excess, are not."""
    POS = np.arange(1, 41) * 7
    L = len(POS)
    paint = np.r_[np.ones(20), 2 * np.ones(20)].astype(np.int32)
    a, b = np.triu_indices(L, 1)
    ln = orc.circ_len(POS[b].astype(float), POS[a].astype(float), float(G))
    a, b = a[ln < 100], b[ln < 100]
    md = np.full((2, 99), np.nan)
    md[0] = 0.05
    md[1] = 0.15
    m0 = 0.3
    c1, c2 = paint[b], paint[a]
    k = np.arange(len(a)) % 3
    low = 0.07 + 0.001 * (np.arange(len(a)) % 50)
    mi = np.where((c1 == c2) & (k == 0), m0, low)
    mi = np.where((c1 == 2) & (c2 == 2) & (k == 1), np.nextafter(m0, 0), mi)
    shape = np.array([[0.4, 60.0], [0.4, 60.0]])
    cut = float(np.sqrt(ref_srp(np.array([0.15]), 0.4, 60.0)[0] * ref_srp(np.array([0.25]), 0.4, 60.0)[0]))
    red, _ = _stage_case(engine, POS, paint, a, b, mi, 100.0, md, shape, cut)
    assert len(red["row"]) > 5 and red["MI"].min() == m0 and (red["clust_c"] == 1).all()
    pa, pb, pm = engine.sr_pool()
    assert ((pm == m0) & (paint[pa] == 2)).sum() > 5 and (pm < m0).sum() == 0
    assert ((mi == np.nextafter(m0, 0))).sum() > 5


@pytest.mark.gpu
def test_nothing_kept_and_tiny_tables(engine):
    """No row kept (n_red 0, NaN minimum, empty pool and flags), a table of 0 rows and of 1 row."""
    POS = np.arange(1, 11) * 10
    paint = np.ones(10, dtype=np.int32)
    md = np.full((1, 99), 0.05)
    a, b = np.array([0, 1, 2]), np.array([3, 4, 5])
    _stage_case(engine, POS, paint, a, b, np.array([0.06, 0.07, 0.04]), 100.0, md, SH3[:1], 1e6)
    _stage_case(engine, POS, paint, E32, E32, E64, 100.0, md, SH3[:1], 1.0)
    for m, cut in ((0.3, 1.0), (0.3, 1e6), (0.01, -1.0)):
        _stage_case(engine, POS, paint, [2], [7], [m], 100.0, md, SH3[:1], cut)
    _place(engine, POS, paint, E32, E32, E64)
    engine.sr_len_quantiles(1, 100.0, 0.95)
    assert np.array_equal(engine.sr_excess_stats(md), np.zeros((1, 5)))
    assert engine.sr_pvalues(md, _shape3(SH3[:1]), 1.0)[:2] == (0, 0)


# ------------------------------------------------------------------------------------------------------------------------------
# GPU: excess statistics, cluster counts and sizes
# ------------------------------------------------------------------------------------------------------------------------------
def _np_stats(a, b, mi, POS, paint, g, sr_dist, md):
    nclust, S = md.shape
    ln = orc.circ_len(np.asarray(POS)[b].astype(float), np.asarray(POS)[a].astype(float), float(g))
    valid = (ln > 0) & (ln < sr_dist)
    li = np.where(valid, ln, 1).astype(np.int64)
    out = np.zeros((nclust, 5))
    c1, c2 = np.asarray(paint)[b], np.asarray(paint)[a]
    for c, extra in ((c1, None), (c2, c1 != c2)):
        e = np.where(valid & (li <= S), mi - md[c - 1, np.minimum(li, S) - 1], np.nan)
        m = e > 0
        if extra is not None:
            m &= extra
        for ci in range(1, nclust + 1):
            x = e[m & (c == ci)]
            out[ci - 1] += [len(x), x.sum(), (x * x).sum(), np.log(x).sum(), np.log1p(-x).sum()]
    return out


def _stats_match(stats, a, b, mi, POS, paint, g, sr_dist, md):
    want = _np_stats(a, b, mi, POS, paint, g, sr_dist, md)
    assert np.array_equal(stats[:, 0], want[:, 0])
    np.testing.assert_allclose(stats, want, rtol=1e-12, atol=1e-300)


def _with_env(name, fn):
    os.environ[name] = "1"
    try:
        return fn()
    finally:
        os.environ.pop(name)


@pytest.mark.gpu
@pytest.mark.parametrize("nclust", [1, 4, 5, 6, 255])
def test_stats_and_pvalues_by_cluster_count(engine, nclust):
    """k_sr_stats_small (nclust <= 4) and the peeling k_sr_stats against numpy, both kernels for every count; then p-values, cut and pool.
    255 clusters (SRM_MAXCL) at a small sr_dist."""
    rng = np.random.default_rng(nclust)
    sr_dist = 40.0 if nclust == 255 else 300.0
    S = int(np.ceil(sr_dist)) - 1
    L = 2 * nclust + 200 if nclust == 255 else 300
    POS = np.sort(rng.choice(np.arange(1, 5 * L), L, replace=False))
    paint = (1 + np.arange(L) % nclust)[rng.permutation(L)].astype(np.int32)
    a, b, mi = _decay_table(rng, POS, paint, 20_000, sr_dist, float(G), w=8 if nclust == 255 else 20)
    md = _md(nclust, S, S, level=0.03)
    md[:, S - S // 3:] = np.nan
    shape = np.column_stack([0.3 + 0.01 * (np.arange(nclust) % 50), 20.0 + np.arange(nclust)])
    _place(engine, POS, paint, a, b, mi)
    engine.sr_len_quantiles(nclust, sr_dist, 0.95)
    stats = engine.sr_excess_stats(md)
    peel = _with_env("LDW_SR_STATS_PEEL", lambda: engine.sr_excess_stats(md))
    _stats_match(stats, a, b, mi, POS, paint, G, sr_dist, md)
    _stats_match(peel, a, b, mi, POS, paint, G, sr_dist, md)
    assert (stats[:, 0] > 0).sum() >= min(nclust, 200)
    _stage_case(engine, POS, paint, a, b, mi, sr_dist, md, shape, 2.0)


@pytest.mark.gpu
def test_stats_blocks_with_empty_and_one_row_blocks(engine):
    rng = np.random.default_rng(7)
    L = 400
    POS = np.sort(rng.choice(np.arange(1, 3000), L, replace=False))
    for nclust in (3, 6):
        paint = rng.integers(1, nclust + 1, L).astype(np.int32)
        a, b, mi = _decay_table(rng, POS, paint, 30_000, 200.0, float(G), w=40)
        md = _md(nclust, 199, 150, level=0.03)
        n = len(a)
        blocks = np.array([0, 1, 0, 5000, 1, 0, 1, n - 5003, 0])
        _place(engine, POS, paint, a, b, mi)
        engine.sr_len_quantiles(nclust, 200.0, 0.95)
        one = engine.sr_excess_stats(md)
        parts = engine.sr_excess_stats_blocks(md, blocks)
        assert parts.shape == (len(blocks), nclust, 5)
        np.testing.assert_allclose(parts.sum(axis=0), one, rtol=1e-12)
        ends = np.cumsum(blocks)
        for k in range(len(blocks)):
            s = slice(ends[k] - blocks[k], ends[k])
            if blocks[k] == 0:
                assert (parts[k] == 0).all()
            else:
                _stats_match(parts[k], a[s], b[s], mi[s], POS, paint, G, 200.0, md)
        _stats_match(one, a, b, mi, POS, paint, G, 200.0, md)


@pytest.mark.gpu
def test_stats_blocks_through_the_peeling_kernel_at_a_small_cluster_count(engine):
    """ldw_sr_excess_stats_blocks at nclust <= 4 under LDW_SR_STATS_PEEL: the peeling k_sr_stats over segments cut into strips, where
    k_sr_stats_small is the default.  Blocks of 0, 1 and 70 rows (fewer rows than strips x 2: empty strips), each block against numpy."""
    rng = np.random.default_rng(12)
    L, nclust = 400, 3
    POS = np.sort(rng.choice(np.arange(1, 3000), L, replace=False))
    paint = rng.integers(1, nclust + 1, L).astype(np.int32)
    a, b, mi = _decay_table(rng, POS, paint, 30_000, 200.0, float(G), w=40)
    md = _md(nclust, 199, 150, level=0.03)
    blocks = np.array([0, 1, 5000, 0, 70, len(a) - 5071])
    _place(engine, POS, paint, a, b, mi)
    engine.sr_len_quantiles(nclust, 200.0, 0.95)
    parts = _with_env("LDW_SR_STATS_PEEL", lambda: engine.sr_excess_stats_blocks(md, blocks))
    assert parts.shape == (len(blocks), nclust, 5) and (paint[a] != paint[b]).sum() > 1000
    ends = np.cumsum(blocks)
    for k in range(len(blocks)):
        s = slice(ends[k] - blocks[k], ends[k])
        if blocks[k] == 0:
            assert (parts[k] == 0).all()
        else:
            _stats_match(parts[k], a[s], b[s], mi[s], POS, paint, G, 200.0, md)
    _stats_match(parts.sum(axis=0), a, b, mi, POS, paint, G, 200.0, md)


@pytest.mark.gpu
def test_past_the_row_floor_and_the_grid_stride():
    """About 5 M kept rows and pool rows on a fresh engine: more than the 2^22-row floor of ldw_sr_pvalues' outputs (the second pass runs)
    and than 16384 x 256 (k_sr_pval / k_sr_pool stride round), and than 2048 x 256 (k_sr_stats' strips hold several rows per lane)."""
    from ldweaver_amd.engine import Engine
    rng = np.random.default_rng(8)
    L, n, sr_dist = 4000, 5_000_000, 1000.0
    POS = np.arange(1, L + 1) * 3
    paint = np.where(rng.random(L) < 0.05, 2, 1).astype(np.int32)     # (a tenth of the rows cross clusters)
    a = rng.integers(0, L - 300, n).astype(np.int32)
    b = (a + rng.integers(1, 300, n)).astype(np.int32)
    md = _md(2, 999, 999, level=2.0 ** -8)
    mi = md[0, 0] + rng.uniform(1e-4, 0.6, n)
    shape = np.array([[0.6, 8.0], [1.3, 5.0]])
    with Engine(0) as eng:
        _place(eng, POS, paint, a, b, mi)
        eng.sr_len_quantiles(2, sr_dist, 0.95)
        _stats_match(eng.sr_excess_stats(md), a, b, mi, POS, paint, G, sr_dist, md)
        n_red, n_pool, mn = eng.sr_pvalues(md, _shape3(shape), -1.0)
        assert n_red == n_pool > (1 << 22) and n_red > 16384 * 256
        red = eng.sr_reduced()
        pa, pb, pm = eng.sr_pool()
        o = np.argsort(red["row"])
        want, _ = np_sr_reduce(a, b, mi, POS, paint, G, sr_dist, md, shape, -1.0)
        w = np.argsort(want["row"])
        for k in ("row", "clust_c", "first_clust", "dup"):
            assert np.array_equal(red[k][o], want[k][w]), k
        np.testing.assert_allclose(red["srp_max"][o], want["srp_max"][w], rtol=2e-10, atol=1e-13)
        assert np.array_equal(red["MI"][o], mi[want["row"][w]]) and mn == mi[want["row"]].min()
        po = np.lexsort((pm, pb, pa))
        wr = np.sort(want["row"])
        wo = np.lexsort((mi[wr], b[wr], a[wr]))
        assert np.array_equal(pa[po], a[wr][wo]) and np.array_equal(pb[po], b[wr][wo]) and np.array_equal(pm[po], mi[wr][wo])


# ------------------------------------------------------------------------------------------------------------------------------
# GPU: end to end against the oracle's mergeNsort_sr_links + runARACNE
# ------------------------------------------------------------------------------------------------------------------------------
def _e2e_case(engine, POS, paint, a, b, mi, nclust, sr_dist, min_rows=30, g=G):
    POS, paint = np.asarray(POS), np.asarray(paint)
    _place(engine, POS, paint, a, b, mi, g)
    tab = _oracle_table(a, b, mi, POS, paint, g)
    # a cut-off in a wide gap of the oracle's srp_max: the two beta optimisers agree to ~1e-6, far inside it
    probe, _ = orc.merge_n_sort_sr_links(_by_clust(tab, nclust), nclust, sr_dist, -1e300)
    s = np.unique(np.asarray(probe["srp_max"]))
    s = s[int(0.4 * len(s)): int(0.8 * len(s))]
    gi = int(np.argmax(np.diff(s)))
    assert s[gi + 1] - s[gi] > 1e-4 * s[gi + 1]
    cut = 0.5 * (s[gi] + s[gi + 1])
    ored, ochk = orc.merge_n_sort_sr_links(_by_clust(tab, nclust), nclust, sr_dist, cut)
    oflags = orc.run_aracne(ored["pos1"], ored["pos2"], ored["MI"], ochk["pos1"], ochk["pos2"], ochk["MI"])
    osrp = np.asarray(ored["srp_max"])
    for order_links in (False, True):
        red, flags, aux = SRP.merge_n_sort_sr_links_device(engine, nclust, sr_dist, cut, POS, paint, float(g), run_aracne=True,
                                                           order_links=order_links)
        o = np.argsort(-osrp, kind="stable") if order_links else np.arange(len(osrp))
        if order_links:                 # (an order of the oracle's p-values the 1e-6 of the optimisers cannot change)
            so = osrp[o]
            d = so[:-1] - so[1:]
            assert ((d == 0) | (d > 1e-5 * so[:-1])).all()
        got = dict(pos1=POS[red["b"]], pos2=POS[red["a"]], clust1=paint[red["b"]], clust2=paint[red["a"]], MI=red["MI"], clust_c=red["clust_c"])
        assert len(red["MI"]) == len(osrp) >= min_rows
        for k, v in got.items():
            assert np.array_equal(np.asarray(v, dtype=float), np.asarray(ored[k], dtype=float)[o]), (order_links, k)
        assert np.abs(red["srp_max"] - osrp[o]).max() < 1e-6 * max(1.0, float(np.abs(osrp).max()))
        assert np.array_equal(flags, oflags[o]), (order_links, int((flags != oflags[o]).sum()))
    assert 0 < oflags.sum() < len(oflags) and (np.asarray(ored["clust1"]) != np.asarray(ored["clust2"])).any()
    return ored


@pytest.mark.gpu
def test_end_to_end_many_clusters_and_ties(engine):
    rng = np.random.default_rng(9)
    L, sr_dist = 400, 300.5
    POS = np.sort(rng.choice(np.arange(1, 3000), L, replace=False))
    paint = rng.integers(1, 6, L).astype(np.int32)
    a, b, mi = _decay_table(rng, POS, paint, 25_000, sr_dist, float(G))
    a, b, mi = _plant_triangles(rng, POS, a, b, mi, 30)
    ored = _e2e_case(engine, POS, paint, a, b, mi, 5, sr_dist)
    assert (np.asarray(ored["clust1"]) != np.asarray(ored["clust2"])).sum() > 20


@pytest.mark.gpu
def test_end_to_end_repeated_positions(engine):
    """Positions held by two SNPs: same-position rows (len 0) leave the model on both sides and never reach the pool; twins with the same
    cluster and MI make cross-cluster keys held by two rows."""
    rng = np.random.default_rng(11)
    L, sr_dist = 300, 400.0
    POS = _twin_positions(rng, L)
    paint = rng.integers(1, 4, L).astype(np.int32)
    tw = np.r_[False, POS[1:] == POS[:-1]]
    paint[tw] = paint[np.nonzero(tw)[0] - 1]
    a, b, mi = _decay_table(rng, POS, paint, 15_000, sr_dist, float(G))
    a, b, mi = _twin_rows(POS, paint, *_plant_triangles(rng, POS, a, b, mi, 20))
    same = np.nonzero(tw)[0]
    a = np.r_[a, same - 1].astype(np.int32)                  # same-position rows with a high MI
    b = np.r_[b, same].astype(np.int32)
    mi = np.r_[mi, np.full(len(same), 0.9)]
    assert (POS[a] == POS[b]).sum() >= 50
    _e2e_case(engine, POS, paint, a, b, mi, 3, sr_dist)
