"""GPU: the kernels of ldw_mi_score_scan and ldw_mi_score_links as functions (ldw_debug_score_scan, ldw_debug_score_links; pytest -m gpu) against the numpy
statement tests/scoresel_ref.py, on values no alignment produces and at every edge of their geometry: patches of 64 rows x 256 columns, four waves of 64
columns in batches of 16.  The two sides are compared apart; counts with array_equal, scores bit for bit, the list as a set, the partners exactly."""
import ctypes as C

import numpy as np
import pytest

import decay_ref as D
import scoresel_ref as S
from ldweaver_amd import _lib as L

pytestmark = pytest.mark.gpu

G = 100000
THR = 2.0 ** -3 + 2.0 ** -30                      # a value of the inputs: with w = 0 the score of such a pair equals the threshold
EDGES = D.bucket_lo(np.array([1, 2, 128, 129, 1000, 2561, 4095]))
SPECIAL = np.concatenate([[0.0, -0.0, -1.0, -1e-300, 5e-324, -5e-324, 1e-310, -1e-310, np.nan, np.inf, -np.inf, 3.0, 1.6, 2.0 ** -20, D.below(2.0 ** -20), THR, D.below(THR)],
                          EDGES, D.below(EDGES)])


def values(rng, shape):
    """A third special values (signed zeros, negatives, subnormals, NaN, infinities, bucket edges and the doubles below them, the threshold and the double
    below it), the rest log-uniform."""
    v = np.exp(rng.uniform(-16, 1, shape))
    pick = rng.random(shape) < 0.35
    v[pick] = rng.choice(SPECIAL, int(pick.sum()))
    return v


def ascending(rng, n, lo=1, hi=G):
    return np.sort(rng.integers(lo, hi + 1, n)).astype(np.int32)


def ids(rng, nf, nt, diag):
    """Global ids that are not in positional order; a diagonal block has one set."""
    p = rng.permutation(5000)
    return (p[:nf], p[:nf]) if diag else (p[:nf], p[nf:nf + nt])


def check(engine, mi, pf, pt, g, diag, sr, wf, wt, idf, idt, thr=THR, masks=(1, 2, 3)):
    """Both kernels equal the statement under every mask: histogram, bests, pair and NaN counts; the list as a set with its exact count; the partners from
    the scan's own bests.  Returns the scan and the links of the last mask."""
    for mask in masks:
        ref = S.scan(mi, pf, pt, g, diag, sr, mask, wf, wt)
        got = engine.debug_score_scan(mi, pf, pt, g, diag, sr, mask, wf, wt)
        assert got["hist"].dtype == np.uint64 and np.array_equal(got["hist"], ref["hist"]), (mask, np.flatnonzero(got["hist"] != ref["hist"])[:5])
        assert S.same_bits(got["best_f"], ref["best_f"]), (mask, "rows", np.flatnonzero(got["best_f"].view(np.int64) != ref["best_f"].view(np.int64))[:5])
        assert S.same_bits(got["best_t"], ref["best_t"]), (mask, "cols", np.flatnonzero(got["best_t"].view(np.int64) != ref["best_t"].view(np.int64))[:5])
        assert got["npairs"] == ref["npairs"] and got["stats"][1] == ref["nan"] and int(got["hist"].sum()) + ref["nan"] == ref["npairs"], (mask, got["npairs"], got["stats"])
        rl, rpf, rpt = S.links(mi, pf, pt, g, diag, sr, mask, idf, idt, wf, wt, thr, ref["best_f"], ref["best_t"])
        n = engine.debug_score_links(mi, pf, pt, g, diag, sr, mask, idf, idt, wf, wt, thr)             # cap = 0 with null lists: a pure count
        assert n["count"] == len(rl) and n["a"] is None and n["partner_f"] is None
        lk = engine.debug_score_links(mi, pf, pt, g, diag, sr, mask, idf, idt, wf, wt, thr, len(rl), got["best_f"], got["best_t"])
        assert lk["count"] == len(rl) and lk["stats"][1] == ref["nan"] and lk["stats"][0] == got["stats"][0]
        if len(rl):
            listed = set(zip(lk["a"].tolist(), lk["b"].tolist(), lk["mi"].view(np.int64).tolist(), lk["score"].view(np.int64).tolist()))
            assert len(listed) == len(rl) and listed == rl, (mask, sorted(listed ^ rl)[:5])
        assert lk["partner_f"].dtype == np.int32 and np.array_equal(lk["partner_f"], rpf), (mask, "rows", np.flatnonzero(lk["partner_f"] != rpf)[:5])
        assert np.array_equal(lk["partner_t"], rpt), (mask, "cols", np.flatnonzero(lk["partner_t"] != rpt)[:5])
        assert np.array_equal(lk["partner_f"] < 0, np.isnan(ref["best_f"])) and np.array_equal(lk["partner_t"] < 0, np.isnan(ref["best_t"]))
    return ref, rl, lk


OFF_SHAPES = [(1, 1), (1, 300), (300, 1)] + [(nf, nt) for nf in (63, 64, 65) for nt in (255, 256, 257)] + [(130, 600)]


@pytest.mark.parametrize("nf,nt", OFF_SHAPES)
def test_off_diagonal_shapes(engine, nf, nt):
    """Positions spread over the circle with sr_dist 5000, weights of mixed signs: long-range patches, short-range patches and mixed ones."""
    rng = np.random.default_rng(1000 * nf + nt)
    idf, idt = ids(rng, nf, nt, False)
    ref, rl, _ = check(engine, values(rng, (nf, nt)), ascending(rng, nf), ascending(rng, nt), G, False, 5000.0, rng.uniform(-0.4, 0.4, nf), rng.uniform(-0.4, 0.4, nt),
                       idf, idt)
    assert ref["npairs"] == nf * nt - min(nf, nt)
    if (nf, nt) == (1, 1):
        assert np.isnan(ref["best_f"]).all() and np.isnan(ref["best_t"]).all() and not rl
    else:
        assert rl and ref["nan"] > 0


@pytest.mark.parametrize("n", (1, 2, 64, 65, 130, 300))
def test_diagonal_shapes(engine, n):
    rng = np.random.default_rng(77 * n)
    p = ascending(rng, n, 1, 20000)
    w = rng.uniform(-0.4, 0.4, n)
    idf, _ = ids(rng, n, n, True)
    ref, _, lk = check(engine, values(rng, (n, n)), p, p, G, True, 3000.0, w, w, idf, idf)
    assert ref["npairs"] == n * (n - 1) // 2
    if n == 1:
        assert lk["stats"][0] == 0 and np.isnan(ref["best_f"]).all()


def test_zero_weights_leave_the_values_bucket_edges_and_the_threshold_are_closed(engine):
    """w = 0: s = mi - 0 keeps every bit, the sign of a zero included, so the special values are the scores: a score at a bucket edge counts in the bucket, the
    double below it in the one below; a score equal to thr is listed, the double below it is not."""
    rng = np.random.default_rng(5)
    nf, nt = 65, 257
    mi = rng.choice(SPECIAL, (nf, nt))
    idf, idt = ids(rng, nf, nt, False)
    ref, rl, lk = check(engine, mi, ascending(rng, nf), ascending(rng, nt), G, False, 5000.0, np.zeros(nf), np.zeros(nt), idf, idt, masks=(3,))
    m = D.pair_mask(nf, nt, False)
    ok = m & ~np.isnan(mi)
    assert np.array_equal(ref["hist"], np.bincount(D.mi_bucket(mi[ok]), minlength=4096))
    for e in EDGES:
        B = int(D.mi_bucket(np.array([e]))[0])
        assert ref["hist"][B] >= (ok & (mi == e)).sum() > 0 and ref["hist"][B - 1] >= (ok & (mi == D.below(e))).sum() > 0
    with np.errstate(invalid="ignore"):
        assert len(rl) == (m & (mi >= THR)).sum() and (m & (mi == THR)).sum() > 0 and (m & (mi == D.below(THR))).sum() > 0
    bits = set(np.array([THR]).view(np.int64).tolist())
    assert bits <= {t[3] for t in rl} and not set(np.array([D.below(THR)]).view(np.int64).tolist()) & {t[3] for t in rl}
    assert ref["nan"] == (m & np.isnan(mi)).sum() > 0


def test_a_weight_that_makes_every_score_negative(engine):
    rng = np.random.default_rng(6)
    nf, nt = 66, 300
    mi = np.exp(rng.uniform(-16, 1, (nf, nt)))
    idf, idt = ids(rng, nf, nt, False)
    ref, rl, lk = check(engine, mi, ascending(rng, nf), ascending(rng, nt), G, False, 5000.0, np.full(nf, 50.0), np.full(nt, 60.0), idf, idt, thr=0.0, masks=(3,))
    assert not rl and lk["count"] == 0 and ref["hist"][0] == ref["npairs"] and (ref["best_f"] < 0).all() and (ref["best_t"] < 0).all()
    assert (lk["partner_f"] >= 0).all() and (lk["partner_t"] >= 0).all()       # the best is still defined, and so is its partner


def test_best_ties_between_the_zeros_and_between_partners(engine):
    """Scores -0 and +0 only (w = 0): +0 is the larger, a row or column of -0 alone keeps its sign; among the partners that tie for the best the smallest id
    wins, with ids that are not in positional order."""
    rng = np.random.default_rng(8)
    nf, nt = 66, 258
    mi = np.where(rng.random((nf, nt)) < 0.5, 0.0, -0.0)
    mi[5, :] = -0.0
    mi[:, 7] = -0.0
    idf, idt = ids(rng, nf, nt, False)
    ref, _, lk = check(engine, mi, ascending(rng, nf, 1, 2000), ascending(rng, nt, 40000, 60000), G, False, 5000.0, np.zeros(nf), np.zeros(nt), idf, idt, masks=(2,))
    assert np.signbit(ref["best_f"][5]) and np.signbit(ref["best_t"][7]) and not np.signbit(ref["best_f"][6])
    plus = ~np.signbit(mi[6]) & (np.arange(nt) != 6)
    assert plus.sum() > 50 and lk["partner_f"][6] == idt[plus].min()           # the smallest id among the +0 partners, wherever it stands
    assert lk["partner_f"][5] == np.delete(idt, 5).min()                       # every partner ties at -0
    mi2 = rng.choice(np.array([0.25, 0.5]), (nf, nt))                          # two values: about half the partners of a SNP tie for its best
    check(engine, mi2, ascending(rng, nf), ascending(rng, nt), G, False, 5000.0, np.zeros(nf), np.zeros(nt), idf, idt)


def test_best_in_nan_and_best_in_that_matches_nothing(engine):
    rng = np.random.default_rng(9)
    nf, nt = 65, 257
    mi = np.exp(rng.uniform(-16, 1, (nf, nt)))
    pf, pt, wf, wt = ascending(rng, nf), ascending(rng, nt), rng.uniform(0, 0.3, nf), rng.uniform(0, 0.3, nt)
    idf, idt = ids(rng, nf, nt, False)
    sc = S.scan(mi, pf, pt, G, False, 5000.0, 3, wf, wt)
    bf, bt = sc["best_f"].copy(), sc["best_t"].copy()
    bf[::3], bt[::5] = np.nan, np.nan
    bf[1::3], bt[1::5] = 123.456, -0.0                                          # scores no pair has
    _, rpf, rpt = S.links(mi, pf, pt, G, False, 5000.0, 3, idf, idt, wf, wt, np.inf, bf, bt)
    lk = engine.debug_score_links(mi, pf, pt, G, False, 5000.0, 3, idf, idt, wf, wt, np.inf, 0, bf, bt)
    assert lk["count"] == 0 and np.array_equal(lk["partner_f"], rpf) and np.array_equal(lk["partner_t"], rpt)
    assert (lk["partner_f"][::3] == -1).all() and (lk["partner_f"][1::3] == -1).all() and (lk["partner_f"][2::3] >= 0).all()
    assert (lk["partner_t"][::5] == -1).all() and (lk["partner_t"][1::5] == -1).all() and (lk["partner_t"][2::5] >= 0).all()


def test_the_masks_on_a_patch_astride_sr_dist_with_pairs_exactly_at_it(engine):
    rng = np.random.default_rng(11)
    nf, nt = 64, 256
    pf, pt = ascending(rng, nf, 1, 3000), ascending(rng, nt, 1, 6000)
    ln = D.circ_len(pt[None, :], pf[:, None], G)
    m = D.pair_mask(nf, nt, False)
    sr = float(np.median(ln[m]))                                               # the len of some pair
    assert (ln == sr).any()
    mi, wf, wt = values(rng, (nf, nt)), rng.uniform(-0.4, 0.4, nf), rng.uniform(-0.4, 0.4, nt)
    idf, idt = ids(rng, nf, nt, False)
    n = {}
    for mask in (1, 2, 3):
        n[mask] = check(engine, mi, pf, pt, G, False, sr, wf, wt, idf, idt, masks=(mask,))[0]["npairs"]
    assert n[1] == (m & (ln <= sr)).sum() > 0 and n[2] == (m & (ln > sr)).sum() > 0 and n[3] == n[1] + n[2]      # len == sr_dist is short range


def test_a_patch_across_the_origin(engine):
    rng = np.random.default_rng(12)
    g = 10000
    pf = np.sort(rng.integers(g - 300, g + 1, 64)).astype(np.int32)            # the from side ends the circle, the to side begins it
    pt = np.sort(rng.integers(1, 300, 256)).astype(np.int32)
    mi, wf, wt = values(rng, (64, 256)), rng.uniform(-0.4, 0.4, 64), rng.uniform(-0.4, 0.4, 256)
    idf, idt = ids(rng, 64, 256, False)
    ref, _, _ = check(engine, mi, pf, pt, g, False, 600.0, wf, wt, idf, idt, masks=(2,))       # every pair within 600 across the origin: none is long range
    assert ref["npairs"] == 0 and np.isnan(ref["best_f"]).all()
    check(engine, mi, pf, pt, g, False, 250.0, wf, wt, idf, idt)


@pytest.mark.parametrize("order", ("shuffled", "one_position"))
def test_position_orders_and_sr_dist_zero_and_infinite(engine, order):
    rng = np.random.default_rng(14 + len(order))
    nf, nt = 130, 600
    pf, pt = rng.permutation(ascending(rng, nf)), rng.permutation(ascending(rng, nt))
    if order == "one_position":
        pf, pt = np.full(nf, 4242, dtype=np.int32), np.full(nt, 4242, dtype=np.int32)
    mi, wf, wt = values(rng, (nf, nt)), rng.uniform(-0.4, 0.4, nf), rng.uniform(-0.4, 0.4, nt)
    idf, idt = ids(rng, nf, nt, False)
    ref, _, _ = check(engine, mi, pf, pt, G, False, np.inf, wf, wt, idf, idt, masks=(1, 2))
    assert ref["npairs"] == 0                                                   # +inf: no pair is long range
    ref, _, _ = check(engine, mi, pf, pt, G, False, 0.0, wf, wt, idf, idt, masks=(2, 1))
    ln = D.circ_len(pt[None, :], pf[:, None], G)
    assert ref["npairs"] == (D.pair_mask(nf, nt, False) & (ln == 0)).sum() and (order != "one_position" or ref["npairs"] == nf * nt - nf)


def raw_links(engine, mi, pf, pt, g, diag, sr, mask, idf, idt, wf, wt, thr, cap, room, with_lists=True):
    """ldw_debug_score_links straight through ctypes, the four lists ``room`` entries long and filled with a guard value."""
    nf, nt = mi.shape
    mf = np.asfortranarray(mi)
    a, b = np.full(room, -7, dtype=np.int32), np.full(room, -7, dtype=np.int32)
    mo, sc = np.full(room, -7.0), np.full(room, -7.0)
    n = C.c_int64(-1)
    ptr = (lambda x: L.ptr(x) if with_lists else None)
    pf, pt, idf, idt = (np.ascontiguousarray(x, dtype=np.int32) for x in (pf, pt, idf, idt))      # (named: they must outlive the call)
    wf, wt = np.ascontiguousarray(wf, dtype=np.float64), np.ascontiguousarray(wt, dtype=np.float64)
    rc = L.lib().ldw_debug_score_links(engine._ctx, L.ptr(mf), nf, nt, L.ptr(pf), L.ptr(pt), float(g), int(diag), float(sr), mask, L.ptr(idf), L.ptr(idt), L.ptr(wf), L.ptr(wt),
                                       float(thr), None, None, cap, ptr(a), ptr(b), ptr(mo), ptr(sc), C.byref(n), None, None, None)
    return rc, int(n.value), a, b, mo, sc


def test_a_cap_below_the_count_and_a_pure_count(engine):
    rng = np.random.default_rng(17)
    nf, nt = 130, 600
    mi = np.exp(rng.uniform(-6, 1, (nf, nt)))
    pf, pt, wf, wt = ascending(rng, nf), ascending(rng, nt), rng.uniform(0, 0.3, nf), rng.uniform(0, 0.3, nt)
    idf, idt = ids(rng, nf, nt, False)
    rl, _, _ = S.links(mi, pf, pt, G, False, 5000.0, 3, idf, idt, wf, wt, 0.5)
    total = len(rl)
    assert total > 2000
    for cap in (1, 100, total - 1):
        rc, n, a, b, mo, sc = raw_links(engine, mi, pf, pt, G, False, 5000.0, 3, idf, idt, wf, wt, 0.5, cap, cap + 4096)
        assert rc == L.LDW_ERR_SIZE and n == total                              # the count stays exact
        assert (a[cap:] == -7).all() and (b[cap:] == -7).all() and (mo[cap:] == -7.0).all() and (sc[cap:] == -7.0).all()      # nothing past cap
        with pytest.raises(L.LdwError) as e:
            engine.debug_score_links(mi, pf, pt, G, False, 5000.0, 3, idf, idt, wf, wt, 0.5, cap)
        assert e.value.code == L.LDW_ERR_SIZE and e.value.count == total
    rc, n, a, b, mo, sc = raw_links(engine, mi, pf, pt, G, False, 5000.0, 3, idf, idt, wf, wt, 0.5, total, total + 4096)
    assert rc == L.LDW_OK and n == total and (a[total:] == -7).all() and (sc[total:] == -7.0).all()
    assert set(zip(a[:total].tolist(), b[:total].tolist(), mo[:total].view(np.int64).tolist(), sc[:total].view(np.int64).tolist())) == rl
    rc, n, *_ = raw_links(engine, mi, pf, pt, G, False, 5000.0, 3, idf, idt, wf, wt, 0.5, 0, 1, with_lists=False)      # cap = 0 with null lists
    assert rc == L.LDW_OK and n == total
    rc, n, *_ = raw_links(engine, mi, pf, pt, G, False, 5000.0, 3, idf, idt, wf, wt, np.nan, 0, 1, with_lists=False)   # a NaN threshold lists nothing
    assert rc == L.LDW_OK and n == 0


@pytest.mark.parametrize("bad", ("w_inf", "w_nan", "mask_0", "mask_4", "sr_negative", "sr_nan", "diag", "g", "lists", "partner_without_best", "id"))
def test_refusals(engine, bad):
    mi, pf, pt = np.ones((4, 5)), np.arange(4, dtype=np.int32), np.arange(5, dtype=np.int32)
    wf, wt, idf, idt = np.zeros(4), np.zeros(5), np.arange(4, dtype=np.int32), np.arange(5, dtype=np.int32) + 4
    sr, mask, diag, g = 10.0, 3, False, 100.0
    if bad == "w_inf":
        wt[3] = np.inf
    elif bad == "w_nan":
        wf[2] = np.nan
    elif bad.startswith("mask"):
        mask = int(bad[-1])
    elif bad == "sr_negative":
        sr = -1.0
    elif bad == "sr_nan":
        sr = np.nan
    elif bad == "diag":
        diag = True
    elif bad == "g":
        g = 0.0
    elif bad == "id":
        idt[1] = -1
    if bad not in ("lists", "partner_without_best", "id"):
        with pytest.raises(L.LdwError) as e:
            engine.debug_score_scan(mi, pf, pt, g, diag, sr, mask, wf, wt)
        assert e.value.code == L.LDW_ERR_ARG
        if bad == "w_inf":
            assert "w_t[3]" in str(e.value)                                    # the message names the index
    if bad == "lists":
        rc, *_ = raw_links(engine, mi, pf, pt, g, diag, sr, mask, idf, idt, wf, wt, 0.0, 3, 8, with_lists=False)
        assert rc == L.LDW_ERR_ARG
    elif bad == "partner_without_best":
        n, part = C.c_int64(0), np.zeros(5, dtype=np.int32)
        mf, part4 = np.asfortranarray(mi), np.zeros(4, dtype=np.int32)
        rc = L.lib().ldw_debug_score_links(engine._ctx, L.ptr(mf), 4, 5, L.ptr(pf), L.ptr(pt), g, 0, sr, mask, L.ptr(idf), L.ptr(idt), L.ptr(wf), L.ptr(wt),
                                           0.0, None, None, 0, None, None, None, None, C.byref(n), L.ptr(part4), L.ptr(part), None)
        assert rc == L.LDW_ERR_ARG
    else:
        with pytest.raises(L.LdwError) as e:
            engine.debug_score_links(mi, pf, pt, g, diag, sr, mask, idf, idt, wf, wt, 0.0)
        assert e.value.code == L.LDW_ERR_ARG
    o = engine.debug_score_scan(np.ones((4, 5)), pf, pt, 100.0, False, 10.0, 3, np.zeros(4), np.zeros(5))      # the context stays usable
    assert o["npairs"] == 16 and o["hist"][D.mi_bucket(np.array([1.0]))[0]] == 16
