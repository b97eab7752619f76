"""GPU: the kernels of ldw_mi_segment_map and ldw_mi_segment_best as functions (ldw_debug_segment_map, ldw_debug_segment_best; pytest -m gpu) against the
numpy statement tests/segmap_ref.py, on values no alignment produces and at every edge of their geometry: patches of 64 rows x 256 columns, four waves of
64 columns, a window of 8 row runs x 16 column runs.  Routes 0, 1 and 2 must give the same bytes: integers with array_equal, maxima and best pairs bit
for bit."""
import numpy as np
import pytest

import decay_ref as D
import segmap_ref as G
from ldweaver_amd import _lib as L

pytestmark = pytest.mark.gpu

GEN = 100000
THR = 2.0 ** -3 + 2.0 ** -30                      # a value of the inputs: with w = None such a pair equals the threshold
U = 2.0 ** -40
SPECIAL = np.array([0.0, -0.0, -1.0, -1e-300, 5e-324, -5e-324, 1e-310, -1e-310, np.nan, np.inf, -np.inf, 3.0, 1.6, THR, D.below(THR),
                    0.5 * U, 1.5 * U, 2.5 * U, -0.5 * U, -1.5 * U, -2.5 * U,                  # the half-way cases of q, even and odd k, both signs
                    2.0 ** -16 - U, 1.0 + 2.0 ** -16 - U, -(2.0 ** -16) - U, -U, -1.0 - U,      # q with all 24 low bits set; negative q
                    D.below(4.0), 4.0, -D.below(4.0), -4.0])                                    # the doubles on both sides of 4


def values(rng, shape):
    """A third special values, the rest log-uniform."""
    v = np.exp(rng.uniform(-16, 1, shape))
    pick = rng.random(shape) < 0.35
    v[pick] = rng.choice(SPECIAL, int(pick.sum()))
    return v


def ascending(rng, n, lo=1, hi=GEN):
    return np.sort(rng.integers(lo, hi + 1, n)).astype(np.int32)


def runs(n, starts, ids):
    """seg (n,): run k starts at starts[k] (starts[0] == 0; starts past n are dropped) and carries ids[k]."""
    seg = np.empty(n, dtype=np.int32)
    for k, s in enumerate(starts):
        if s < n:
            seg[s:] = ids[k]
    return seg


def patches(nf, nt, diag):
    """Patches the kernel visits: all of them, but a diagonal block's patches wholly on or above the diagonal."""
    return sum(1 for a0 in range(0, nf, 64) for b0 in range(0, nt, 256) if not diag or min(a0 + 64, nf) - 1 > b0)


def ids_of(rng, nf, nt, diag):
    p = rng.permutation(5000)
    return (p[:nf], p[:nf]) if diag else (p[:nf] + 5000, p[nf:nf + nt])        # from-ids above to-ids off the diagonal


def check(engine, mi, pf, pt, g, diag, sf, st, S, sr, mask, wf=None, wt=None, thr=THR, idf=None, idt=None, routes=(0, 1, 2)):
    """Both kernels equal the statement under every route asked for; returns the statement's map, the route-0 result and its best pairs."""
    nf, nt = mi.shape
    if idf is None:
        idf, idt = (np.arange(nf), np.arange(nf)) if diag else (np.arange(nf) + nt, np.arange(nt))
    ref = G.segment_map(mi, pf, pt, g, diag, sf, st, S, sr, mask, wf, wt, thr)
    rbest = G.segment_best(mi, pf, pt, g, diag, sf, st, S, sr, mask, idf, idt, ref["max"], wf, wt)
    out = None
    for route in routes:
        got = engine.debug_segment_map(mi, pf, pt, g, diag, sf, st, S, sr, mask, wf, wt, thr, route)
        for k in G.INTS:
            assert got[k].dtype == np.int64 and np.array_equal(got[k], ref[k]), (route, k, np.argwhere(got[k] != ref[k])[:5])
        assert G.same_bits(got["max"], ref["max"]), (route, np.argwhere(got["max"].view(np.int64) != ref["max"].view(np.int64))[:5])
        assert got["npairs"] == ref["npairs"] == int(got["n"].sum()), (route, got["npairs"], ref["npairs"])
        st4 = got["stats"]
        assert st4[0] == patches(nf, nt, diag) and st4[2] == ref["refused"] and st4[3] == ref["nan"], (route, st4, ref["refused"], ref["nan"])
        assert st4[1] == (st4[0] if route == 2 else 0 if route == 1 else st4[1])
        b = engine.debug_segment_best(mi, pf, pt, g, diag, sf, st, S, sr, mask, idf, idt, got["max"], wf, wt, route)
        assert b["pair"].dtype == np.uint64 and np.array_equal(b["pair"], rbest), (route, np.argwhere(b["pair"] != rbest)[:5])
        assert b["stats"][0] == st4[0] and b["stats"][1] == st4[1] and b["stats"][3] == ref["nan"]
        if route == 0 or out is None:
            out = (got, b["pair"])
    # a cell has a best pair exactly where it has a maximum
    assert np.array_equal(rbest != G.NO_PAIR, ~np.isnan(ref["max"]))
    return ref, out[0], out[1]


ROW_STARTS = (0, 1, 63, 64, 65)
COL_STARTS = (0, 63, 64, 65, 127, 128, 191, 192, 255, 256, 257)              # the wave-chunk edges and the patch edges
OFF_SHAPES = [(1, 1), (1, 300), (300, 1)] + [(nf, nt) for nf in (63, 64, 65) for nt in (255, 256, 257)] + [(130, 600)]


@pytest.mark.parametrize("nf,nt", OFF_SHAPES)
def test_off_diagonal_shapes_with_runs_at_every_edge(engine, nf, nt):
    """Run boundaries at rows 0/1, 62/63/64/65 and at columns 63/64/65, 127/128, 191/192, 255/256/257; from-ids above to-ids: a patch holds at most 3 row
    runs and 9 column runs, so every route applies."""
    rng = np.random.default_rng(1000 * nf + nt)
    S = 20
    sf, st = runs(nf, ROW_STARTS, [15, 16, 17, 18, 19]), runs(nt, COL_STARTS, list(range(11)))
    mi, pf, pt = values(rng, (nf, nt)), ascending(rng, nf), ascending(rng, nt)
    idf, idt = ids_of(rng, nf, nt, False)
    ref, got, _ = check(engine, mi, pf, pt, GEN, False, sf, st, S, 5000.0, 3, idf=idf, idt=idt)
    assert ref["npairs"] == nf * nt - min(nf, nt) and got["stats"][1] == 0        # route 0 stays on route 1
    wf, wt = rng.uniform(-0.4, 0.4, nf), rng.uniform(-0.4, 0.4, nt)
    for mask in (1, 2):
        check(engine, mi, pf, pt, GEN, False, sf, st, S, 30000.0, mask, wf, wt, idf=idf, idt=idt)
    if (nf, nt) != (1, 1):
        assert ref["nan"] > 0 and ref["refused"] > ref["nan"]


@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 130, 300))
def test_diagonal_shapes(engine, n):
    """A diagonal block from one SNP on: one set of segments, same-id cells (s == t) on and off the block's diagonal patches."""
    rng = np.random.default_rng(77 * n)
    p = ascending(rng, n, 1, 20000)
    seg = runs(n, (0, 1, 40, 64, 100, 256, 257), [3, 0, 3, 1, 0, 2, 3])      # ids repeat: one id in two runs of a patch and in two patches
    w = rng.uniform(-0.4, 0.4, n)
    idf, _ = ids_of(rng, n, n, True)
    mi = values(rng, (n, n))
    ref, got, _ = check(engine, mi, p, p, GEN, True, seg, seg, 4, 3000.0, 3, idf=idf, idt=idf)
    assert ref["npairs"] == n * (n - 1) // 2 and got["stats"][1] == 0
    check(engine, mi, p, p, GEN, True, seg, seg, 4, 3000.0, 2, w, w, idf=idf, idt=idf)
    if n == 1:
        assert not ref["n"].any() and np.isnan(ref["max"]).all()
    if n >= 63:
        assert ref["n"][0, 0] > 0 and ref["n"][3, 3] > 0


def test_segment_layouts(engine):
    rng = np.random.default_rng(5)
    nf, nt = 130, 600
    mi, pf, pt = values(rng, (nf, nt)), ascending(rng, nf), ascending(rng, nt)
    one = check(engine, mi, pf, pt, GEN, False, np.zeros(nf, np.int32), np.zeros(nt, np.int32), 1, 5000.0, 3)[0]      # one segment for all
    assert one["n"].shape == (1, 1) and one["n"][0, 0] == nf * nt - nf
    # -1 runs at a patch's start, middle and end, on both sides
    sf = runs(nf, (0, 5, 30, 40, 60, 64, 70), [-1, 2, -1, 2, -1, -1, 1])
    st = runs(nt, (0, 10, 100, 130, 250, 256, 300, 590), [-1, 0, -1, 1, -1, 3, -1, 0])
    ref = check(engine, mi, pf, pt, GEN, False, sf, st, 4, 5000.0, 3)[0]
    assert ref["npairs"] == int(((sf[:, None] >= 0) & (st[None, :] >= 0) & ~np.eye(nf, nt, dtype=bool)).sum()) > 0
    # the same id in two separate runs of one patch and in two patches; descending ids; from-ids above and below to-ids; s == t cells
    sf = runs(nf, (0, 20, 40, 64, 100), [5, 3, 5, 3, 1])
    st = runs(nt, (0, 50, 100, 200, 256, 400, 512), [6, 5, 6, 2, 5, 1, 0])
    ref, got, _ = check(engine, mi, pf, pt, GEN, False, sf, st, 7, 5000.0, 3)
    assert ref["n"][5, 5] > 0 and ref["n"][1, 1] > 0 and ref["n"][3, 5] > 0 and ref["n"][1, 3] > 0 and got["stats"][1] == 0
    # at most 2 row runs x 2 column runs per patch: must stay on route 1
    sf, st = runs(nf, (0, 33, 100), [0, 1, 2]), runs(nt, (0, 200, 300, 520), [3, 4, 5, 6])
    ref, got, _ = check(engine, mi, pf, pt, GEN, False, sf, st, 7, 5000.0, 3)
    assert got["stats"][1] == 0 and got["stats"][0] == 9
    # shuffled ids: more runs than the window holds
    sf, st = rng.integers(-1, 6, nf).astype(np.int32), rng.integers(-1, 6, nt).astype(np.int32)
    ref, got, _ = check(engine, mi, pf, pt, GEN, False, sf, st, 6, 5000.0, 3, routes=(0, 2))
    assert got["stats"][1] == got["stats"][0] == 9
    with pytest.raises(L.LdwError) as e:
        engine.debug_segment_map(mi, pf, pt, GEN, False, sf, st, 6, 5000.0, 3, route=1)
    assert e.value.code == L.LDW_ERR_ARG and "route 1" in str(e.value)
    # 9 row runs (one too many) with one column run; 17 column runs (one too many) with one row run: only these patches leave route 1
    sf9, st1 = runs(nf, tuple(range(0, 63, 7)), list(range(9))), np.zeros(nt, np.int32)
    got = check(engine, mi, pf, pt, GEN, False, sf9, st1, 9, 5000.0, 3, routes=(0, 2))[1]
    assert got["stats"][1] == 3                                                 # the three patches of rows 0..63
    sf1, st17 = np.zeros(nf, np.int32), runs(nt, (0,) + tuple(range(256, 512, 15)), list(range(19)))
    got = check(engine, mi, pf, pt, GEN, False, sf1, st17, 19, 5000.0, 3, routes=(0, 2))[1]
    ncr = 1 + int((np.diff(st17[256:512]) != 0).sum())
    assert ncr > 16 and got["stats"][1] == 3                                    # the three patches of columns 256..511


def test_every_snp_its_own_segment(engine):
    rng = np.random.default_rng(6)
    n = 130
    p = ascending(rng, n, 1, 20000)
    mi = values(rng, (n, n))
    seg = np.arange(n, dtype=np.int32)
    ref, got, pair = check(engine, mi, p, p, GEN, True, seg, seg, n, 3000.0, 3, routes=(0, 2))
    assert got["stats"][1] == got["stats"][0] == patches(n, n, True) and (np.tril(ref["n"].T, -1) == np.tril(np.ones((n, n), np.int64), -1)).all()
    a, b = np.tril_indices(n, -1)
    ok = ~np.isnan(mi[a, b])
    assert G.same_bits(got["max"][b, a][ok], mi[a, b][ok]) and np.isnan(got["max"][b, a][~ok]).all()      # every maximum is the cell's own value
    assert np.array_equal(pair[b, a][ok], (b[ok].astype(np.uint64) << np.uint64(32)) | a[ok].astype(np.uint64))
    with pytest.raises(L.LdwError) as e:
        engine.debug_segment_map(mi, p, p, GEN, True, seg, seg, n, 3000.0, 3, route=1)
    assert e.value.code == L.LDW_ERR_ARG
    off = check(engine, mi[:, :100], p, p[:100], GEN, False, seg, seg[:100] + 30, n, 3000.0, 3, routes=(0, 2))[0]      # shuffled ids too
    perm = rng.permutation(n).astype(np.int32)
    check(engine, mi, p, p, GEN, True, perm, perm, n, 3000.0, 2, routes=(0, 2))
    assert off["npairs"] == n * 100 - 100


def test_planted_values(engine):
    """One cell per question.  Segment 0: the tie of the maximum between -0 and +0; 1: two pairs tied for the maximum; 2: NaN only; 3: the threshold and the
    double below it; 4: the doubles on both sides of 4 and the infinities; 5: q with all 24 low bits set and negative q; 6: subnormals and half-way cases."""
    nf, nt = 8, 14
    mi = np.zeros((nf, nt))
    sf = np.zeros(nf, np.int32)
    st = np.repeat(np.arange(7, dtype=np.int32), 2)
    pf, pt = np.arange(1, nf + 1, dtype=np.int32) * 10, 1000 + np.arange(nt, dtype=np.int32) * 10
    mi[:, 0:2] = -0.0
    mi[3, 1] = 0.0
    mi[:, 2:4] = 0.125
    mi[5, 2] = mi[2, 3] = mi[6, 3] = 0.75
    mi[:, 4:6] = np.nan
    mi[:, 6] = THR
    mi[:, 7] = D.below(THR)
    mi[:, 8] = [D.below(4.0), 4.0, -D.below(4.0), -4.0, np.inf, -np.inf, 3.0, 1.0]
    mi[:, 9] = 1.0
    mi[:, 10] = [2.0 ** -16 - U, 1.0 + 2.0 ** -16 - U, -(2.0 ** -16) - U, -U, -1.0 - U, -3.0, 2.0 ** -16, -(2.0 ** -16)]
    mi[:, 11] = -0.25
    mi[:, 12] = [5e-324, -5e-324, 1e-310, 0.5 * U, 1.5 * U, 2.5 * U, -0.5 * U, -1.5 * U]
    mi[:, 13] = [-2.5 * U, 3.5 * U, -3.5 * U, 0.25 * U, 0.75 * U, -0.75 * U, U, -U]
    mi[0, 0] = mi[1, 1] = 7.0                                                   # the local diagonal of an off-diagonal block: no pair
    idf, idt = np.arange(nf) + 100, np.arange(nt)
    ref, got, pair = check(engine, mi, pf, pt, GEN, False, sf, st, 7, 100.0, 3, idf=idf, idt=idt)
    mx = got["max"][0]
    assert mx[0] == 0.0 and not np.signbit(mx[0])                               # +0 above -0
    assert pair[0, 0] == (1 << 32) | 103                                        # the only +0
    assert mx[1] == 0.75 and pair[0, 1] == (2 << 32) | 105                      # the smaller packed pair of the three tied: (2, 105) < (3, 102) < (3, 106)
    # (columns 0..7 lose their local-diagonal pair: 2 nf - 2 pairs in each of the first four cells)
    assert got["n"][0, 2] == 2 * nf - 2 and np.isnan(mx[2]) and pair[0, 2] == G.NO_PAIR and got["nge"][0, 2] == 0 and got["stats"][3] == 2 * nf - 2
    assert got["nge"][0, 3] == nf - 1 and got["n"][0, 3] == 2 * nf - 2          # a value equal to thr counts, the double below it does not
    assert mx[4] == np.inf and got["n"][0, 4] == 2 * nf and got["nge"][0, 4] == 2 * nf - 3      # the refused values still count in n, nge and max
    assert got["stats"][2] == 2 * nf - 2 + 4                                    # NaN, 4, -4 and the infinities are refused; the doubles inside 4 are not
    py_q = lambda cols: sum(round(float(v) * 2.0 ** 40) for v in mi[:, cols].ravel())      # Python's integers and round(): half to even on an exact scaling
    ex = G.exact(got)
    assert round(D.below(4.0) * 2.0 ** 40) == 2 ** 42 and ex[0, 4] == (3 << 40) + (1 << 40) + nf * (1 << 40)
    assert ex[0, 5] == py_q([10, 11]) == (-3 << 40) - (1 << 41) + (1 << 24) - 5 and got["sum_lo"][0, 5] == 5 * (2 ** 24 - 1) and got["sum_hi"][0, 5] < 0
    assert ex[0, 6] == py_q([12, 13]) == (0 + 0 + 0 + 0 + 2 + 2 + 0 - 2) + (-2 + 4 - 4 + 0 + 1 - 1 + 1 - 1)      # ties to even; subnormals round to 0
    none = engine.debug_segment_map(mi, pf, pt, GEN, False, sf, st, 7, 100.0, 3, thr=np.inf)
    assert none["nge"].sum() == none["nge"][0, 4] == 1 and np.array_equal(none["n"], got["n"])      # +inf counts no finite value (inf >= inf is an fp64 truth)
    nanthr = engine.debug_segment_map(mi, pf, pt, GEN, False, sf, st, 7, 100.0, 3, thr=np.nan)
    assert not nanthr["nge"].any()


def test_geometry(engine):
    rng = np.random.default_rng(9)
    nf, nt = 70, 300
    mi = values(rng, (nf, nt))
    sf, st = runs(nf, (0, 30, 64), [0, 1, 2]), runs(nt, (0, 100, 256), [2, 3, 0])
    # pairs exactly at sr_dist: rows at 1000 + k, columns at 1500 + k: many pairs at 500 exactly, under every mask
    pf, pt = (1000 + np.arange(nf)).astype(np.int32), (1500 + np.arange(nt) % 40).astype(np.int32)      # repeated positions on the to side
    maps = [check(engine, mi, pf, pt, GEN, False, sf, st, 4, 500.0, mask)[0] for mask in (1, 2, 3)]
    at = (pt[None, :] - pf[:, None] == 500) & ~np.eye(nf, nt, dtype=bool)
    assert at.sum() > 0 and np.array_equal(maps[0]["n"] + maps[1]["n"], maps[2]["n"]) and maps[0]["npairs"] >= at.sum()
    below = check(engine, mi, pf, pt, GEN, False, sf, st, 4, D.below(500.0), 1)[0]
    assert maps[0]["npairs"] - below["npairs"] == at.sum()                       # closed at sr_dist
    # a patch across the origin, reversed positions
    pf2 = ((GEN - 35 + np.arange(nf)) % GEN + 1).astype(np.int32)
    pt2 = ((GEN - 150 + np.arange(nt)[::-1]) % GEN + 1).astype(np.int32)
    for mask in (1, 2):
        m = check(engine, mi, pf2, pt2, GEN, False, sf, st, 4, 60.0, mask)[0]
        assert m["npairs"] > 0
    # a fractional g; sr_dist 0 and +inf
    gf = 99999.5
    for sr, mask, n in ((0.0, 1, None), (0.0, 2, None), (np.inf, 1, nf * nt - nf), (np.inf, 2, 0), (7.25, 1, None)):
        m = check(engine, mi, pf2, pt2, gf, False, sf, st, 4, sr, mask)[0]
        assert n is None or m["npairs"] == n
    same = (np.arange(nf) * 3 + 1).astype(np.int32)                              # sr_dist 0: only the pairs of equal positions are short range
    m = check(engine, mi[:, :nf], same, same[::-1].copy(), GEN, False, sf, sf, 4, 0.0, 1)[0]
    assert m["npairs"] == (nf - 1 if nf % 2 else nf)                           # a == nf - 1 - b, but the local diagonal


def test_weights_against_none(engine):
    rng = np.random.default_rng(10)
    nf, nt = 65, 257
    mi, pf, pt = values(rng, (nf, nt)), ascending(rng, nf), ascending(rng, nt)
    sf, st = runs(nf, (0, 10), [1, 0]), runs(nt, (0, 100, 256), [0, 1, 2])
    plain = check(engine, mi, pf, pt, GEN, False, sf, st, 3, 5000.0, 3)[1]
    zero = check(engine, mi, pf, pt, GEN, False, sf, st, 3, 5000.0, 3, np.zeros(nf), np.zeros(nt))[1]
    assert all(np.array_equal(plain[k], zero[k]) for k in G.INTS) and G.same_bits(plain["max"], zero["max"])      # mi - 0 * 0 is mi, -0 included
    wf, wt = rng.uniform(-0.4, 0.4, nf), rng.uniform(-0.4, 0.4, nt)
    other = check(engine, mi, pf, pt, GEN, False, sf, st, 3, 5000.0, 3, wf, wt)[1]
    assert not np.array_equal(other["sum_lo"], plain["sum_lo"]) and np.array_equal(other["n"], plain["n"])
    lean = engine.debug_segment_map(mi, pf, pt, GEN, False, sf, st, 3, 5000.0, 3)        # the nullable outputs
    import ctypes as C
    n, npairs = np.zeros((3, 3), np.int64), C.c_int64(0)
    mf = np.asfortranarray(mi)
    L.check(L.lib().ldw_debug_segment_map(engine._ctx, L.ptr(mf), nf, nt, L.ptr(pf), L.ptr(pt), float(GEN), 0, L.ptr(sf), L.ptr(st), 3, 5000.0, 3, None, None, THR, 0,
                                          L.ptr(n), None, None, None, None, C.byref(npairs), None))
    assert np.array_equal(n, lean["n"]) and npairs.value == lean["npairs"]


def test_every_refusal(engine):
    mi, p, q, s2, s3 = np.zeros((2, 3)), np.array([1, 2], np.int32), np.array([5, 6, 7], np.int32), np.zeros(2, np.int32), np.zeros(3, np.int32)
    w2, w3 = np.zeros(2), np.zeros(3)

    def bad(match=None, **kw):
        a = dict(mi=mi, pos_f=p, pos_t=q, g=100.0, diag=False, seg_f=s2, seg_t=s3, S=1, sr_dist=5.0, cls_mask=3, w_f=None, w_t=None, thr=0.0, route=0)
        a.update(kw)
        with pytest.raises(L.LdwError) as e:
            engine.debug_segment_map(**a)
        assert e.value.code == L.LDW_ERR_ARG and "ldw_debug_segment_map" in str(e.value) and (match is None or match in str(e.value)), str(e.value)
        b = {k: v for k, v in a.items() if k != "thr"}
        with pytest.raises(L.LdwError) as e:
            engine.debug_segment_best(id_f=np.arange(mi.shape[0]) if "mi" not in kw else np.arange(kw["mi"].shape[0]),
                                      id_t=np.arange(mi.shape[1]) if "mi" not in kw else np.arange(kw["mi"].shape[1]), max_in=np.zeros((1, 1)) if 1 <= b["S"] <= 8192 else np.zeros(1), **b)
        assert e.value.code == L.LDW_ERR_ARG and "ldw_debug_segment_best" in str(e.value)

    bad("S 0", S=0)
    bad("S 8193", S=8193)
    bad("seg_t[2]", seg_t=np.array([0, 0, 1], np.int32))                        # the first bad index is named
    bad("seg_f[1]", seg_f=np.array([0, -2], np.int32))
    bad("sr_dist", sr_dist=-1.0)
    bad("sr_dist", sr_dist=np.nan)
    bad("cls_mask", cls_mask=0)
    bad("cls_mask", cls_mask=4)
    bad("w_f[1]", w_f=np.array([0.0, np.inf]), w_t=w3)
    bad("w_t[0]", w_f=w2, w_t=np.array([np.nan, 0.0, 0.0]))
    bad("both or neither", w_f=w2)
    bad("route", route=3)
    bad("g must", g=0.0)
    bad("diag", diag=True)                                                      # a diagonal block is square
    with pytest.raises(L.LdwError) as e:                                        # an id outside its range
        engine.debug_segment_best(mi, p, q, 100.0, False, s2, s3, 1, 5.0, 3, np.array([0, -1]), np.arange(3), np.zeros((1, 1)))
    assert e.value.code == L.LDW_ERR_ARG and "id_f[1]" in str(e.value)
    ok = engine.debug_segment_map(mi, p, q, 100.0, False, s2 - 1, s3, 1, 5.0, 3)      # every from-SNP at -1: legal, nothing takes part
    assert ok["npairs"] == 0 and not ok["n"].any() and np.isnan(ok["max"]).all()
    big = engine.debug_segment_map(mi, p, q, 100.0, False, s2 + 1023, s3, 1024, 5.0, 3)      # a wide map: the far corner of row 0
    assert big["n"][0, 1023] == 4 and big["n"].sum() == 4
