"""GPU: the kernel of ldw_mi_snp_summary as a function (ldw_debug_snp_summary; pytest -m gpu) against the numpy statement tests/snpsum_ref.py, on values
no alignment produces and at every edge of its geometry: patches of 64 rows x 256 columns, four waves of 64 columns in batches of 16, the single-class route
and the general one.  The row side and the column side are compared apart: integers with array_equal, the maxima bit for bit, on every route."""
import numpy as np
import pytest

import decay_ref as D
import snpsum_ref as R
from ldweaver_amd import _lib as L

pytestmark = pytest.mark.gpu

G = 100000
THR = (2.0 ** -3 + 2.0 ** -30, 2.0 ** -7)          # the thresholds of nge: both are values of the inputs


def above(x):
    return np.nextafter(np.asarray(x, dtype=np.float64), np.inf)


HALVES = np.array([(k + 0.5) * 2.0 ** -40 for k in (0, 1, 2, 3, 1000, 1001, 2 ** 38, 2 ** 38 + 1)])     # exact half-way cases, even and odd k
BEYOND = np.array([2.0 ** 22, -2.0 ** 22, above(2.0 ** 22), np.inf, -np.inf, np.nan, 1e300])            # q refuses these
SPECIAL = np.concatenate([[0.0, -0.0, -1.0, -1e-300, 5e-324, -5e-324, 1e-310, -1e-310, 2.0 ** -41, above(2.0 ** -41), D.below(2.0 ** -41), -2.0 ** -41],
                          HALVES, -HALVES, [THR[0], D.below(THR[0]), THR[1], D.below(THR[1]), D.below(2.0 ** 22), -D.below(2.0 ** 22), 3.0, 1.6]])


def values(rng, shape, beyond=True):
    """A third special values (signed zeros, negatives, subnormals, half-way cases of the fixed point, the thresholds and the doubles just below them, both
    sides of 2^22, infinities and NaN), the rest log-uniform."""
    v = np.exp(rng.uniform(-16, 1, shape))
    pick = rng.random(shape) < 0.35
    v[pick] = rng.choice(np.concatenate([SPECIAL, BEYOND]) if beyond else SPECIAL, int(pick.sum()))
    return v


def check(engine, mi, pf, pt, g, diag, sr, thr=THR, single=None, integral=True):
    """Routes 0 and 2 equal the statement, side by side; route 1 equals it where the bound puts every patch in one class and answers LDW_ERR_ARG where
    it does not."""
    rows, cols, npairs, refused = R.snp_summary(mi, pf, pt, g, diag, sr, thr)
    got = {}
    for route in (0, 2):
        o = engine.debug_snp_summary(mi, pf, pt, g, diag, sr, thr, route)
        for name, side, ref in (("rows", o["rows"], rows), ("cols", o["cols"], cols)):
            for k in ("n", "sumq", "nge"):
                assert side[k].dtype == np.int64 and np.array_equal(side[k], ref[k]), (route, name, k, np.argwhere(side[k] != ref[k])[:5])
            assert R.same_bits(side["max"], ref["max"]), (route, name, side["max"], ref["max"])
        assert np.array_equal(o["npairs"], npairs), (route, o["npairs"], npairs)
        assert np.array_equal(o["rows"]["n"].sum(axis=1), npairs) and np.array_equal(o["cols"]["n"].sum(axis=1), npairs)
        assert o["stats"][3] == refused, (route, o["stats"], refused)
        if integral:
            assert o["stats"][2] == 0                                          # integral g: no pair off its patch's class
        got[route] = o
    assert got[2]["stats"][1] == got[2]["stats"][0]                             # forced: every patch with a pair carried both classes
    all_single = got[0]["stats"][1] == 0
    if single is not None:
        assert all_single == single, (got[0]["stats"], single)
    if all_single:
        o = engine.debug_snp_summary(mi, pf, pt, g, diag, sr, thr, 1)
        assert R.same_side(o["rows"], rows) and R.same_side(o["cols"], cols) and np.array_equal(o["npairs"], npairs) and o["stats"][1] == 0
    else:
        with pytest.raises(L.LdwError) as e:
            engine.debug_snp_summary(mi, pf, pt, g, diag, sr, thr, 1)
        assert e.value.code == L.LDW_ERR_ARG
    return got[0]


def ascending(rng, n, lo=1, hi=G):
    return np.sort(rng.integers(lo, hi + 1, n)).astype(np.int32)


OFF_SHAPES = [(1, 1), (1, 300), (300, 1)] + [(nf, nt) for nf in (63, 64, 65) for nt in (255, 256, 257)] + [(130, 600)]


@pytest.mark.parametrize("nf,nt", OFF_SHAPES)
def test_off_diagonal_shapes(engine, nf, nt):
    """Positions spread over the circle with sr_dist 5000: long-range patches, short-range patches and mixed ones."""
    rng = np.random.default_rng(1000 * nf + nt)
    o = check(engine, values(rng, (nf, nt)), ascending(rng, nf), ascending(rng, nt), G, False, 5000.0)
    assert o["npairs"].sum() == nf * nt - min(nf, nt)
    if (nf, nt) == (1, 1):
        assert not o["rows"]["n"].any() and not o["cols"]["n"].any() and np.isnan(o["rows"]["max"]).all() and np.isnan(o["cols"]["max"]).all()


@pytest.mark.parametrize("n", (1, 2, 64, 65, 130, 300))
def test_diagonal_shapes(engine, n):
    rng = np.random.default_rng(77 * n)
    p = ascending(rng, n, 1, 20000)
    o = check(engine, values(rng, (n, n)), p, p, G, True, 3000.0)
    assert o["npairs"].sum() == n * (n - 1) // 2
    if n == 1:
        assert o["stats"][0] == 0 and np.isnan(o["rows"]["max"]).all()


def test_one_class_patches_take_the_single_route(engine):
    rng = np.random.default_rng(3)
    mi = values(rng, (130, 600))
    o = check(engine, mi, ascending(rng, 130, 1, 2000), ascending(rng, 600, 40000, 60000), G, False, 5000.0, single=True)     # all long range
    assert o["npairs"][0] == 0
    o = check(engine, mi, ascending(rng, 130, 1, 2000), ascending(rng, 600, 1, 2000), G, False, 5000.0, single=True)          # all short range
    assert o["npairs"][1] == 0 and not o["rows"]["n"][1].any() and np.isnan(o["cols"]["max"][1]).all()


def test_rounding_is_to_nearest_even(engine):
    """Every value an exact half-way case (k + 0.5) 2^-40, positive and negative: the sums are those of the even neighbours."""
    rng = np.random.default_rng(5)
    mi = rng.choice(np.concatenate([HALVES, -HALVES]), (65, 257))
    q, ref = R.q_fixed(mi)
    assert not ref.any() and np.array_equal(q[mi > 0] % 2, np.zeros((mi > 0).sum())) and R.q_fixed(np.array([0.5, 1.5, 2.5, -0.5, -1.5]) * 2.0 ** -40)[0].tolist() == [0, 2, 2, 0, -2]
    o = check(engine, mi, ascending(rng, 65), ascending(rng, 257), G, False, 5000.0)
    assert o["stats"][3] == 0


def test_thresholds_are_closed_and_infinity_counts_nothing(engine):
    rng = np.random.default_rng(6)
    nf, nt = 64, 256
    mi = rng.choice(np.array([THR[0], D.below(THR[0]), THR[1], D.below(THR[1]), np.nan]), (nf, nt))
    pf, pt = ascending(rng, nf, 1, 2000), ascending(rng, nt, 1, 2000)
    o = check(engine, mi, pf, pt, G, False, 5000.0, single=True)               # every pair short range: thr[0] alone applies
    m = D.pair_mask(nf, nt, False)
    with np.errstate(invalid="ignore"):
        assert o["rows"]["nge"][0].sum() == (m & (mi >= THR[0])).sum() == (m & (mi == THR[0])).sum() > 0
    o = check(engine, np.exp(rng.uniform(-16, 1, (nf, nt))), pf, pt, G, False, 5000.0, thr=(np.inf, np.inf))
    assert not o["rows"]["nge"].any() and not o["cols"]["nge"].any()


def test_maximum_ties_between_the_zeros(engine):
    """Values -0 and +0 only: +0 is the larger; a row or column of -0 alone keeps its sign."""
    rng = np.random.default_rng(8)
    mi = np.where(rng.random((66, 258)) < 0.5, 0.0, -0.0)
    mi[5, :] = -0.0
    mi[:, 7] = -0.0
    o = check(engine, mi, ascending(rng, 66, 1, 2000), ascending(rng, 258, 40000, 60000), G, False, 5000.0, single=True)
    assert np.signbit(o["rows"]["max"][1][5]) and np.signbit(o["cols"]["max"][1][7]) and not np.signbit(o["rows"]["max"][1][6])
    assert not o["rows"]["sumq"].any()


def test_values_beyond_the_fixed_point_add_zero_and_are_counted(engine):
    rng = np.random.default_rng(9)
    nf, nt = 65, 257
    mi = rng.choice(np.concatenate([BEYOND, [D.below(2.0 ** 22), -D.below(2.0 ** 22), 0.5]]), (nf, nt))
    o = check(engine, mi, ascending(rng, nf), ascending(rng, nt), G, False, 5000.0)
    m = D.pair_mask(nf, nt, False)
    with np.errstate(invalid="ignore"):
        assert o["stats"][3] == (m & ~(np.abs(mi) < 2.0 ** 22)).sum() > 0
    assert np.isnan(o["rows"]["max"][o["rows"]["n"] > 0]).any()                 # a NaN orders above +inf


def test_a_patch_astride_sr_dist_and_pairs_exactly_at_it(engine):
    rng = np.random.default_rng(11)
    nf, nt = 64, 256
    pf, pt = ascending(rng, nf, 1, 3000), ascending(rng, nt, 1, 6000)
    ln = D.circ_len(pt[None, :], pf[:, None], G)
    sr = float(np.median(ln[D.pair_mask(nf, nt, False)]))                      # the len of some pair
    assert (ln == sr).any()
    o = check(engine, values(rng, (nf, nt)), pf, pt, G, False, sr, single=False)
    assert o["npairs"][0] == (D.pair_mask(nf, nt, False) & (ln <= sr)).sum() and o["npairs"][0] > 0 and o["npairs"][1] > 0


def test_a_patch_across_the_origin_and_len_at_half_the_circle(engine):
    rng = np.random.default_rng(12)
    g = 10000
    pf = np.sort(rng.integers(g - 300, g + 1, 64)).astype(np.int32)            # the from side ends the circle, the to side begins it
    pt = np.sort(rng.integers(1, 300, 256)).astype(np.int32)
    mi = values(rng, (64, 256))
    o = check(engine, mi, pf, pt, g, False, 600.0, single=True)                # every pair within 600 across the origin
    assert o["npairs"][1] == 0
    check(engine, mi, pf, pt, g, False, 250.0, single=False)
    pf2 = ascending(rng, 66, 1, g // 2)
    pt2 = (pf2 + g // 2).astype(np.int32)
    pt2[:3] = pf2[3:6] + g // 2                                                 # pairs (3, 0), (4, 1), (5, 2) exactly opposite: len = g / 2
    mi2 = values(rng, (66, 66))
    ln = D.circ_len(pt2[None, :], pf2[:, None], g)
    assert (ln[D.pair_mask(66, 66, False)] == g / 2).sum() >= 3
    o = check(engine, mi2, pf2, pt2, g, False, g / 2.0)                        # len == sr_dist is short range: every pair is
    assert o["npairs"][1] == 0
    o = check(engine, mi2, pf2, pt2, g, False, g / 2.0 - 1)
    assert o["npairs"][1] == (D.pair_mask(66, 66, False) & (ln > g / 2 - 1)).sum() >= 3


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
    elif order == "repeated":                                                  # runs of five SNPs at one position, the same positions on both sides: many len 0
        runs = np.repeat(pf[::5], 5)
        pf, pt = np.resize(runs, nf).astype(np.int32), np.resize(runs, nt).astype(np.int32)
    else:
        pf, pt = np.full(nf, 4242, dtype=np.int32), np.full(nt, 4242, dtype=np.int32)
    if diag:
        pt = pf
    mi = values(rng, (nf, nt))
    o = check(engine, mi, pf, pt, G, diag, 5000.0)
    if order == "one_position":
        assert o["npairs"][1] == 0
    if order in ("repeated", "one_position"):
        o = check(engine, mi, pf, pt, G, diag, 0.0)                            # sr_dist 0: short range is len == 0 alone
        ln = D.circ_len(pt[None, :], pf[:, None], G)
        assert o["npairs"][0] == (D.pair_mask(nf, nt, diag) & (ln == 0)).sum() > 0


def test_sr_dist_zero_and_infinite(engine):
    rng = np.random.default_rng(14)
    nf, nt = 130, 600
    pf, pt = ascending(rng, nf), ascending(rng, nt)
    mi = values(rng, (nf, nt))
    o = check(engine, mi, pf, pt, G, False, np.inf, single=True)
    assert o["npairs"][1] == 0 and o["npairs"][0] == nf * nt - nf
    o = check(engine, mi, pf, pt, G, False, 0.0)
    ln = D.circ_len(pt[None, :], pf[:, None], G)
    assert o["npairs"][0] == (D.pair_mask(nf, nt, False) & (ln == 0)).sum()


def test_a_fractional_genome_length(engine):
    """g = 100000.25: every len has the fraction 0 or .25 up to the rounding of the reduction, so no len lies within 0.2 of sr_dist = 2500.5 and the
    class of every pair is the same under any rounding.  The count of pairs off their patch's class is printed, not asserted: no input is known that makes
    it positive, so the route-1 path that adds such a pair directly is not exercised here or anywhere."""
    rng = np.random.default_rng(15)
    g, sr = 100000.25, 2500.5
    nf, nt = 130, 600
    pf, pt = rng.integers(1, 100001, nf).astype(np.int32), rng.integers(1, 100001, nt).astype(np.int32)
    pt[:200] = np.sort(rng.integers(1, 6000, 200))
    pf[:64] = np.sort(rng.integers(1, 6000, 64))
    ln = D.circ_len(pt[None, :], pf[:, None], g)
    assert np.abs(ln - sr).min() > 0.2
    o = check(engine, values(rng, (nf, nt)), pf, pt, g, False, sr, integral=False)
    assert o["npairs"][0] > 0 and o["npairs"][1] > 0
    print("pairs off their patch's class:", o["stats"][2])


def test_route_1_on_a_mixed_patch_is_refused(engine):
    rng = np.random.default_rng(16)
    pf, pt = ascending(rng, 64, 1, 3000), ascending(rng, 256, 1, 6000)
    with pytest.raises(L.LdwError) as e:
        engine.debug_snp_summary(values(rng, (64, 256)), pf, pt, G, False, 1500.0, THR, 1)
    assert e.value.code == L.LDW_ERR_ARG
    o = engine.debug_snp_summary(np.ones((4, 5)), np.arange(4), np.arange(5), 100.0, False, 10.0, THR, 1)      # the context stays usable
    assert o["npairs"].tolist() == [16, 0]


@pytest.mark.parametrize("bad", ("sr_negative", "sr_nan", "route", "diag", "g"))
def test_refusals(engine, bad):
    mi, pf, pt = np.ones((4, 5)), np.arange(4, dtype=np.int32), np.arange(5, dtype=np.int32)
    sr, route, diag, g = 10.0, 0, False, 100.0
    if bad == "sr_negative":
        sr = -1.0
    elif bad == "sr_nan":
        sr = np.nan
    elif bad == "route":
        route = 3
    elif bad == "diag":
        diag = True
    else:
        g = 0.0
    with pytest.raises(L.LdwError) as e:
        engine.debug_snp_summary(mi, pf, pt, g, diag, sr, THR, route)
    assert e.value.code == L.LDW_ERR_ARG
