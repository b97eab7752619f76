"""GPU: the histogram kernel of ldw_mi_profile as a function (ldw_debug_profile_hist; pytest -m gpu) against the numpy statement tests/decay_ref.py, on
values no alignment produces and at every edge of its geometry: patches of 64 rows x 256 columns, the LDS window of 8192 counters (route A) and the
wave-aggregated global adds (route B).  Counts are compared with array_equal, the maxima bit for bit.  Inputs hold no NaN and g is integral."""
import numpy as np
import pytest

import decay_ref as R
from ldweaver_amd import _lib as L

pytestmark = pytest.mark.gpu

C_COLS = 256                      # columns of a patch (csrc/ldw_decay.hip DEC_C)
LDS_COUNTERS = 8192               # route A's window
OFF_SHAPES = [(1, 1), (1, 2), (2, 1), (63, 3), (64, 3), (65, 3), (3, C_COLS - 1), (3, C_COLS), (3, C_COLS + 1), (129, 257)]
DIAG_SIDES = [1, 2, 64, 65, 129]
G = 100000


def values(rng, shape, shift):
    """Bucket edges and the doubles just below them, at both ends of the range and at multiples of 2^shift; +-0, negatives, 2^-20 and below, 3.0, a
    value past the top; the rest log-uniform."""
    B = np.array([1, 2, 3, 1 << shift, 2 << shift, (1 << shift) + 1, 5 << shift, 2048, 4095 - (1 << shift), 4094, 4095])
    B = B[(B >= 1) & (B <= 4095)]
    edges = R.bucket_lo(B)
    special = np.concatenate([edges, R.below(edges), [0.0, -0.0, -1.0, -1e-300, -3.5, 2.0 ** -20, R.below(2.0 ** -20), 2.0 ** -21, 1e-300, 3.0, 4096.0, 1e6]])
    v = np.exp(rng.uniform(-16, 2, shape))
    pick = rng.random(shape) < 0.35
    v[pick] = rng.choice(special, int(pick.sum()))
    return v


def check(engine, mi, pf, pt, g, diag, cuts, shift, fits=None):
    """Routes 0 and 2 equal the statement; route 1 equals it where every patch fits the window and answers LDW_ERR_ARG where one does not."""
    ref_h, ref_m, ref_n = R.profile_hist(mi, pf, pt, g, diag, cuts, shift)
    got = {}
    for route in (0, 2):
        o = engine.debug_profile_hist(mi, pf, pt, g, diag, cuts, shift, route)
        assert o["hist"].dtype == np.uint64 and o["hist"].shape == ref_h.shape
        assert o["n_pairs"] == ref_n == int(o["hist"].sum()), (route, o["n_pairs"], ref_n)
        assert np.array_equal(o["hist"], ref_h), (route, np.argwhere(o["hist"] != ref_h)[:5])
        assert R.same_max(o["max"], ref_m), (route, o["max"], ref_m)
        assert o["stats"][2] == 0                                          # integral g: no pair outside its patch's bound
        got[route] = o
    assert got[2]["stats"][1] == got[2]["stats"][0]                         # forced: every patch with a pair took route B
    all_fit = got[0]["stats"][1] == 0
    if fits is not None:
        assert all_fit == fits, (got[0]["stats"], fits)
    if all_fit:
        o = engine.debug_profile_hist(mi, pf, pt, g, diag, cuts, shift, 1)
        assert np.array_equal(o["hist"], ref_h) and R.same_max(o["max"], ref_m) and o["stats"][1] == 0
    else:
        with pytest.raises(L.LdwError) as e:
            engine.debug_profile_hist(mi, pf, pt, g, diag, cuts, shift, 1)
        assert e.value.code == L.LDW_ERR_ARG
    return got[0]


def ascending(rng, n, lo=1, hi=G):
    return np.sort(rng.integers(lo, hi + 1, n)).astype(np.int32)


GEO_CUTS = np.unique(np.rint(np.geomspace(100, G / 2, 24, endpoint=False)))


@pytest.mark.parametrize("shift", (0, 3, 6))
@pytest.mark.parametrize("nf,nt", OFF_SHAPES)
def test_off_diagonal_shapes(engine, nf, nt, shift):
    rng = np.random.default_rng(1000 * nf + nt + shift)
    pf, pt = ascending(rng, nf, 1, G // 3), ascending(rng, nt, G // 3 + 1, G)
    o = check(engine, values(rng, (nf, nt), shift), pf, pt, G, False, GEO_CUTS, shift)
    assert o["n_pairs"] == nf * nt - min(nf, nt)
    if (nf, nt) == (1, 1):
        assert o["n_pairs"] == 0 and not o["hist"].any() and np.isnan(o["max"]).all()


@pytest.mark.parametrize("shift", (0, 3, 6))
@pytest.mark.parametrize("n", DIAG_SIDES)
def test_diagonal_shapes(engine, n, shift):
    rng = np.random.default_rng(77 * n + shift)
    p = ascending(rng, n, 1, 20000)
    o = check(engine, values(rng, (n, n), shift), p, p, G, True, GEO_CUTS, shift)
    assert o["n_pairs"] == n * (n - 1) // 2


@pytest.mark.parametrize("order", ("reversed", "shuffled", "repeated", "one_position"))
@pytest.mark.parametrize("diag", (False, True))
def test_position_orders(engine, order, diag):
    rng = np.random.default_rng(10 * len(order) + diag)
    nf, nt = (129, 129) if diag else (130, 300)
    pf, pt = ascending(rng, nf), ascending(rng, nt)
    if order == "reversed":
        pf, pt = pf[::-1].copy(), pt[::-1].copy()
    elif order == "shuffled":
        pf, pt = rng.permutation(pf), rng.permutation(pt)
    elif order == "repeated":                                              # runs of five SNPs at one position, the same positions on both sides: many len 0
        runs = np.repeat(pf[::5], 5)
        pf, pt = np.resize(runs, nf).astype(np.int32), np.resize(runs, nt).astype(np.int32)
    else:
        pf, pt = np.full(nf, 4242, dtype=np.int32), np.full(nt, 4242, dtype=np.int32)
    if diag:
        pt = pf
    o = check(engine, values(rng, (nf, nt), 3), pf, pt, G, diag, GEO_CUTS, 3)
    if order == "one_position":                                            # every len is 0: the first bin holds every pair
        assert o["hist"][0].sum() == o["n_pairs"] and not o["hist"][1:].any()


@pytest.mark.parametrize("shift", (0, 3))
def test_pairs_whose_len_equals_a_cut_belong_to_the_lower_bin(engine, shift):
    rng = np.random.default_rng(5 + shift)
    nf, nt = 70, 260
    pf, pt = ascending(rng, nf, 1, 3000), ascending(rng, nt, 1, 3000)
    ln = R.circ_len(pt[None, :], pf[:, None], G)
    m = R.pair_mask(nf, nt, False)
    cuts = np.unique(rng.choice(ln[m], 40))                                # every cut is the len of some pair
    mi = values(rng, (nf, nt), shift)
    o = check(engine, mi, pf, pt, G, False, cuts, shift)
    for k in (0, len(cuts) // 2, len(cuts) - 1):
        on_cut = m & (ln == cuts[k])
        assert on_cut.any()
        assert o["hist"][k].sum() == (m & (ln <= cuts[k]) & ((ln > cuts[k - 1]) if k else True)).sum()


def test_a_patch_across_the_origin_and_len_at_half_the_circle(engine):
    rng = np.random.default_rng(9)
    g = 10000                                                               # even: len reaches g / 2 exactly
    pf = np.sort(rng.integers(g - 300, g + 1, 64)).astype(np.int32)        # the from side ends the circle, the to side begins it
    pt = np.sort(rng.integers(1, 300, 256)).astype(np.int32)
    cuts = np.array([0.0, 50, 100, 200, 400, 2500, 4999, 5000, 6000])
    o = check(engine, values(rng, (64, 256), 3), pf, pt, g, False, cuts, 3, fits=True)
    assert o["hist"][6:].sum() == 0 and o["hist"][5].sum() > 0              # every pair within 600 across the origin, some beyond 400
    pf2 = ascending(rng, 66, 1, g // 2)
    pt2 = (pf2 + g // 2).astype(np.int32)                                   # the pair (a, a) is no pair; (a, b) has len g / 2 - |p_a - p_b|
    pt2[:3] = pf2[3:6] + g // 2                                             # pairs (3, 0), (4, 1), (5, 2) exactly opposite: len = g / 2
    mi = values(rng, (66, 66), 3)
    o = check(engine, mi, pf2, pt2, g, False, cuts, 3)
    ln = R.circ_len(pt2[None, :], pf2[:, None], g)
    assert (ln[R.pair_mask(66, 66, False)] == g / 2).sum() >= 3
    assert o["hist"][7].sum() == (ln[R.pair_mask(66, 66, False)] > 4999).sum() and not o["hist"][8:].any()   # (4999, 5000] holds them; nothing lies beyond


@pytest.mark.parametrize("shift", (0, 3, 6))
def test_cut_counts_none_one_and_1023(engine, shift):
    rng = np.random.default_rng(20 + shift)
    nf, nt = 65, 257
    pf, pt = ascending(rng, nf), ascending(rng, nt)
    mi = values(rng, (nf, nt), shift)
    o = check(engine, mi, pf, pt, G, False, None, shift, fits=True)        # one distance bin: always fits
    assert o["hist"].shape == (1, 4096 >> shift)
    check(engine, mi, pf, pt, G, False, [2500.0], shift)
    cuts = np.arange(1, 1024) * 48.0                                       # 1023 cuts up to 49 104, just short of g / 2: patches span hundreds of bins
    o = check(engine, mi, pf, pt, G, False, cuts, shift, fits=False)
    assert o["hist"].shape == (1024, 4096 >> shift)


def test_cuts_finer_than_the_snp_spacing(engine):
    """SNPs 40 bp apart, cuts every 2 bp: a patch of 64 x 256 SNPs spans thousands of cuts, so no window fits at any mi_shift, while coarse cuts fit."""
    rng = np.random.default_rng(31)
    nf, nt = 64, 256
    pf = (40 * np.arange(nf) + 1).astype(np.int32)
    pt = (40 * np.arange(nt) + 3000).astype(np.int32)
    fine = np.arange(1, 1024) * 2.0 + 2000
    for shift in (0, 3, 6):
        mi = values(rng, (nf, nt), shift)
        check(engine, mi, pf, pt, G, False, fine, shift, fits=False)
    # the window's edge: 8192 counters hold 16 distance bins at mi_shift 3; the one patch spans len 479 .. 13 199
    assert LDS_COUNTERS // (4096 >> 3) == 16
    mi = values(rng, (nf, nt), 3)
    check(engine, mi, pf, pt, G, False, 400.0 + 1000.0 * np.arange(15), 3, fits=True)       # bins 1 .. 13
    check(engine, mi, pf, pt, G, False, 400.0 + 800.0 * np.arange(17), 3, fits=True)        # bins 1 .. 16: exactly 16
    check(engine, mi, pf, pt, G, False, 400.0 + 790.0 * np.arange(17), 3, fits=False)       # bins 1 .. 17


def test_cuts_all_past_half_the_circle(engine):
    rng = np.random.default_rng(41)
    nf, nt = 100, 300
    o = check(engine, values(rng, (nf, nt), 3), ascending(rng, nf), ascending(rng, nt), G, False, [G / 2 + 1.0, G, 3.0 * G], 3, fits=True)
    assert o["hist"][0].sum() == o["n_pairs"] and not o["hist"][1:].any() and np.isnan(o["max"][1:]).all()


def test_many_patches_add_up(engine):
    """Several patches both ways, mixed routes, the default kind of cuts: what a block of a pass looks like, small."""
    rng = np.random.default_rng(51)
    nf, nt = 331, 777
    p = ascending(rng, 1200, 1, G)
    mi = np.exp(rng.normal(-5, 1.5, (nf, nt)))                              # a smooth population: many lanes share a bucket
    check(engine, mi, p[:nf], p[400:400 + nt], G, False, GEO_CUTS, 3)
    check(engine, mi[:, :nf], p[:nf], p[:nf], G, True, GEO_CUTS, 0)


@pytest.mark.parametrize("bad", ("unsorted", "equal", "nan", "inf", "negative", "n_cut", "shift7", "shift_neg", "route"))
def test_refusals(engine, bad):
    mi, pf, pt = np.ones((4, 5)), np.arange(4, dtype=np.int32), np.arange(5, dtype=np.int32)
    cuts, shift, route = np.array([1.0, 2.0, 3.0]), 3, 0
    if bad == "unsorted":
        cuts = np.array([1.0, 3.0, 2.0])
    elif bad == "equal":
        cuts = np.array([1.0, 2.0, 2.0])
    elif bad == "nan":
        cuts = np.array([1.0, np.nan, 3.0])
    elif bad == "inf":
        cuts = np.array([1.0, 2.0, np.inf])
    elif bad == "negative":
        cuts = np.array([-1.0, 2.0, 3.0])
    elif bad == "n_cut":
        cuts = np.arange(1024) + 1.0
    elif bad == "shift7":
        shift = 7
    elif bad == "shift_neg":
        shift = -1
    else:
        route = 3
    with pytest.raises(L.LdwError) as e:
        engine.debug_profile_hist(mi, pf, pt, 100.0, False, cuts, shift, route)
    assert e.value.code == L.LDW_ERR_ARG
    o = engine.debug_profile_hist(mi, pf, pt, 100.0, False, [1.0, 2.0, 3.0], 3, 0)     # the context stays usable
    assert o["n_pairs"] == 16 and int(o["hist"].sum()) == 16
