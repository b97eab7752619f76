"""The consumers of the link tables — Tukey thresholds (ldw_lr_tukey), ARACNE (ldw_aracne_device) and the LD map (ldw_ldmap) —
against the oracle at the edges a natural MI table almost never reaches: exact ties at a quantile or threshold, tables of a few rows,
the top-links fallback at its boundary, signed zeros and denormals, hubs longer than a wave, grid-stride lengths, SNPs sharing a
position, single-block maps.  Every table is placed with ``Engine.links_import`` (no MI pass); the alignment only satisfies
set_alignment / set_snp_meta.  Large ARACNE cases use ``np_aracne``, a vectorised restatement of runARACNE checked against the
oracle's literal one by a CPU test of this file."""
import re
import warnings

import numpy as np
import pandas as pd
import pytest

import ldw_oracle as orc
from ldweaver_amd import lr as LR
from ldweaver_amd import srp as SRP
from ldweaver_amd.snpdat import SnpDat
from ldweaver_amd.synth import synth_alignment

G = 50_000_000          # genome length of the synthetic cases (positions stay far below it: no wrap-around)
E32 = np.zeros(0, dtype=np.int32)
E64 = np.zeros(0, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------------------
# vectorised runARACNE (R/io_functions.R:101-164) on distinct positions
# ------------------------------------------------------------------------------------------------------------------------------
def np_aracne(chk_a, chk_b, chk_mi, pa, pb, pmi, POS) -> np.ndarray:
    """ARACNE flags of the links (chk_a, chk_b) — SNP indices, a = from side (pos2), b = to side (pos1) — against the pool rows
    (pa, pb, pmi).  Nodes are distinct positions.  Per (node, neighbour) the MI of the first pool row joining them counts (the
    reference's match() into matX / matZ); flag = False iff some common neighbour y has MI(X,Z) < MI(X,y) and MI(X,Z) < MI(Z,y).
    Pool rows joining two SNPs at one position are outside what this restates (they shift the reference's indexing)."""
    POS = np.asarray(POS)
    _, slot = np.unique(POS, return_inverse=True)
    slot = slot.astype(np.int64)
    n = int(slot.max()) + 1 if len(slot) else 1
    pa, pb, pmi = np.asarray(pa, dtype=np.int64), np.asarray(pb, dtype=np.int64), np.asarray(pmi, dtype=np.float64)
    m0 = np.asarray(chk_mi, dtype=np.float64)
    out = np.ones(len(m0), dtype=bool)
    u = np.concatenate([slot[pa], slot[pb]])
    v = np.concatenate([slot[pb], slot[pa]])
    m = np.concatenate([pmi, pmi])
    row = np.concatenate([np.arange(len(pa)), np.arange(len(pa))])
    ok = u != v
    u, v, m, row = u[ok], v[ok], m[ok], row[ok]
    if len(u) == 0 or len(m0) == 0:
        return out
    key = u * n + v
    o = np.lexsort((row, key))
    key, m = key[o], m[o]
    first = np.ones(len(key), dtype=bool)
    first[1:] = key[1:] != key[:-1]
    key, m = key[first], m[first]
    node, nbr = key // n, key % n
    off = np.searchsorted(node, np.arange(n + 1))
    X, Z = slot[np.asarray(chk_b, dtype=np.int64)], slot[np.asarray(chk_a, dtype=np.int64)]
    dx, dz = off[X + 1] - off[X], off[Z + 1] - off[Z]
    S, T = np.where(dx <= dz, X, Z), np.where(dx <= dz, Z, X)     # walk the shorter list, look up in the other
    cnt = off[S + 1] - off[S]
    w = np.repeat(np.arange(len(X)), cnt)
    e = np.arange(int(cnt.sum())) + np.repeat(off[S] - (np.cumsum(cnt) - cnt), cnt)
    q = T[w] * n + nbr[e]
    k = np.minimum(np.searchsorted(key, q), len(key) - 1)
    ind = (key[k] == q) & (m0[w] < m[e]) & (m0[w] < m[k])
    out[w[ind]] = False
    return out


def _random_pool(rng, POS, n_rows, levels):
    """n_rows random links between SNPs at DIFFERENT positions with MI drawn from a few levels (ties everywhere)."""
    L = len(POS)
    a = rng.integers(0, L, 4 * n_rows)
    b = rng.integers(0, L, 4 * n_rows)
    ok = POS[a] != POS[b]
    a, b = a[ok][:n_rows], b[ok][:n_rows]
    assert len(a) == n_rows
    return a.astype(np.int32), b.astype(np.int32), rng.choice(levels, n_rows).astype(np.float64)


@pytest.mark.parametrize("repeated", [False, True])
def test_np_aracne_equals_oracle_aracne(repeated):
    """The vectorised reference of this file against orc.run_aracne (the literal restatement) on random pools with tied MI values,
    unique positions and positions held by two SNPs (no pool row inside one position)."""
    rng = np.random.default_rng(11 + repeated)
    flags = 0
    for trial in range(25):
        L = 60
        if repeated:
            POS = np.repeat(np.sort(rng.choice(np.arange(1, 400), L // 2, replace=False)) * 10, 2)
            if trial % 2:
                POS = POS[rng.permutation(L)]
        else:
            POS = np.sort(rng.choice(np.arange(1, 4000), L, replace=False)) * 10
        pa, pb, pmi = _random_pool(rng, POS, 300, [0.25, 0.375, 0.5, 0.625, 0.75])
        ck = rng.choice(300, 80, replace=False)
        ca, cb, cmi = pa[ck], pb[ck], pmi[ck]
        want = orc.run_aracne(POS[cb], POS[ca], cmi, POS[pb], POS[pa], pmi)
        got = np_aracne(ca, cb, cmi, pa, pb, pmi, POS)
        assert np.array_equal(got, want), trial
        flags += int(want.sum())
    assert 0 < flags < 25 * 80


# ------------------------------------------------------------------------------------------------------------------------------
# the Python layer's argument checks (R/LDSummaryPlot.R:30-47, R/lr_analyser.R:93)
# ------------------------------------------------------------------------------------------------------------------------------
class _MapEngine:
    def __init__(self):
        self.calls = []

    def ldmap(self, reducer, from_, to):
        self.calls.append((reducer, from_, to))
        return np.zeros((1, 1)), 10, reducer


def test_ldmap_argument_checks_match_the_reference():
    eng = _MapEngine()
    with pytest.warns(UserWarning, match=re.escape("<reducer> for genomewide_LDMap should be >0, set to default")):
        LR.genomewide_LDMap(eng, None, reducer=-3)
    assert eng.calls[-1] == (0, 0, 0)           # set to default: the library's reducer 0
    with pytest.raises(ValueError, match=re.escape("If <from> is provided, <to> must be provided as well!")):
        LR.genomewide_LDMap(eng, None, from_=100)
    with pytest.raises(ValueError, match=re.escape("If <to> is provided, <from> must be provided as well!")):
        LR.genomewide_LDMap(eng, None, to=100)
    for f, t in ((100, 100), (200, 100)):
        with pytest.raises(ValueError, match=re.escape("<to> must be greater than <from>!")):
            LR.genomewide_LDMap(eng, None, from_=f, to=t)
    with pytest.raises(ValueError, match=re.escape("<from> and <to> must be positive values")):
        LR.genomewide_LDMap(eng, None, from_=-5, to=100)
    assert len(eng.calls) == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        LR.genomewide_LDMap(eng, None, reducer=0, from_=10.4, to=20.6)   # reducer 0 is no warning; from / to are rounded
    assert eng.calls[-1] == (0, 10, 21)


# ------------------------------------------------------------------------------------------------------------------------------
# GPU: helpers
# ------------------------------------------------------------------------------------------------------------------------------
_ALN = {}


def _meta(engine, POS):
    """An alignment of len(POS) SNPs and the given positions."""
    L = len(POS)
    if L not in _ALN:
        st = np.ascontiguousarray(synth_alignment(L, 16, seed=L)["states"])
        uqe, r = orc.uqe_r(st)
        _ALN[L] = (st, uqe, r)
    st, uqe, r = _ALN[L]
    engine.set_alignment(st)
    engine.set_snp_meta(r, uqe, np.asarray(POS, dtype=np.int32), np.ones(L, dtype=np.int32), float(G))
    return st, uqe, r


def _tukey_numpy(mi, smi, min_links):
    """analyse_long_range_links' thresholds and selections (R/lr_analyser.R:72-109) from orc.quantile7 and numpy counts."""
    q13 = np.array([orc.quantile7(mi, 0.25), orc.quantile7(mi, 0.75)])
    thr = q13[1] + np.array([1.5, 3.0]) * (q13[1] - q13[0])
    fb = False
    if (mi > thr.min()).sum() < min_links and len(mi) >= min_links:
        fb = True
        thr = np.array([orc.quantile7(mi, max(0.0, 1 - (1 / len(mi)) * 4000)), orc.quantile7(mi, max(0.0, 1 - (1 / len(mi)) * 5000))])
    t = thr.min()
    return q13, thr, fb, np.nonzero(mi > t)[0], int((mi > t).sum() + (smi > t).sum())


def _lr_case(engine, POS, lr, sr=(E32, E32, E64), min_links=5000, aracne="oracle"):
    """Tukey + ARACNE of the long-range table lr = (a, b, MI) with the caller's short-range rows sr against the oracle.  aracne:
    'oracle' (orc.analyse_long_range_links with its literal run_aracne), 'numpy' (np_aracne on the same pool) or None (no ARACNE)."""
    POS = np.asarray(POS, dtype=np.int64)
    a, b, mi = (np.asarray(lr[0], dtype=np.int32), np.asarray(lr[1], dtype=np.int32), np.asarray(lr[2], dtype=np.float64))
    sa, sb, smi = (np.asarray(sr[0], dtype=np.int32), np.asarray(sr[1], dtype=np.int32), np.asarray(sr[2], dtype=np.float64))
    _meta(engine, POS)
    engine.links_import(1, a, b, mi)
    engine.links_import(0, E32, E32, E64)
    info = engine.lr_tukey(min_links, sr=(sa, sb, smi))
    q13, thr, fb, rows, n_pool = _tukey_numpy(mi, smi, min_links)
    assert np.array_equal(info["q13"], q13) and np.array_equal(info["thresholds"], thr), (info, q13, thr)
    assert info["fallback"] == fb
    assert info["n_red"] == len(rows) and info["n_pool"] == n_pool
    red = engine.lr_reduced()
    assert np.array_equal(red["row"], rows)                       # table order
    assert np.array_equal(red["a"], a[rows]) and np.array_equal(red["b"], b[rows]) and np.array_equal(red["MI"], mi[rows])
    if aracne is None:
        return info, None
    flags = engine.aracne_device()
    assert len(flags) == len(rows)
    if aracne == "oracle":
        ref = orc.analyse_long_range_links(dict(pos1=POS[b], pos2=POS[a], MI=mi), dict(pos1=POS[sb], pos2=POS[sa], MI=smi), min_links=min_links)
        assert ref["fallback"] == fb and ref["n_pool"] == n_pool and np.array_equal(ref["thresholds"], thr)
        o = np.argsort(-mi[rows], kind="stable")
        assert np.array_equal(rows[o], ref["rows"])
        want = np.empty(len(rows), dtype=bool)
        want[o] = ref["ARACNE"]
    else:
        t = thr.min()
        kl, ks = mi > t, smi > t
        want = np_aracne(a[rows], b[rows], mi[rows], np.concatenate([a[kl], sa[ks]]), np.concatenate([b[kl], sb[ks]]),
                         np.concatenate([mi[kl], smi[ks]]), POS)
    bad = np.nonzero(flags != want)[0]
    assert len(bad) == 0, f"{len(bad)} of {len(want)} ARACNE flags differ from the oracle; first rows {rows[bad[:8]]}"
    return info, flags


def _ascending(L, step=1000):
    return (np.arange(L, dtype=np.int64) + 1) * step


def _filler(rng, L, n, avoid_pos=None):
    """n low-MI long-range rows in [0, 0.01]: they set q1 / q3 far below the planted links and stay out of the pool."""
    a = rng.integers(0, L, 2 * n)
    b = rng.integers(0, L, 2 * n)
    ok = a != b if avoid_pos is None else avoid_pos[a] != avoid_pos[b]
    a, b = a[ok][:n], b[ok][:n]
    return a.astype(np.int32), b.astype(np.int32), rng.uniform(0.0, 0.01, n)


def _cat(*tabs):
    return tuple(np.concatenate([np.asarray(t[k]) for t in tabs]) for k in range(3))


# ------------------------------------------------------------------------------------------------------------------------------
# GPU: Tukey
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 9])
def test_tukey_tiny_tables(engine, n):
    """Type-7 quantile indices integral (n = 1, 5, 9) or interpolated, with distinct, tied and all-equal values."""
    rng = np.random.default_rng(n)
    L = 12
    POS = _ascending(L)
    for values in (rng.permutation(np.arange(1, n + 1) / 8.0), rng.choice([0.25, 0.5, 0.75], n), np.full(n, 0.375),
                   np.r_[np.full(n - 1, 0.125), 4.0][rng.permutation(n)]):
        a = rng.integers(0, L // 2, n)
        b = rng.integers(L // 2, L, n)
        _lr_case(engine, POS, (a, b, values))


@pytest.mark.gpu
def test_tukey_exact_ties_at_quantiles_and_thresholds(engine):
    rng = np.random.default_rng(3)
    L = 40
    POS = _ascending(L)

    def rand_ab(n):
        a = rng.integers(0, L // 2, n)
        return a, a + rng.integers(1, L // 2, n)

    # q1 = 0.25, q3 = 0.5 at integral indices, threshold q3 + 1.5 IQR = 0.875 exactly: 20 rows sit on it (strict >: not kept)
    v = rng.permutation(np.r_[np.full(40, 0.25), np.full(40, 0.5), np.full(20, 0.875), np.full(5, 1.0)])
    info, _ = _lr_case(engine, POS, (*rand_ab(len(v)), v))
    assert info["thresholds"][0] == 0.875 and info["n_red"] == 5
    # q1 == q3 with fractional indices (n = 6: 2.25 and 4.75), IQR 0
    info, _ = _lr_case(engine, POS, (*rand_ab(6), np.array([0.9, 0.3, 0.3, 0.1, 0.3, 0.3])))
    assert info["q13"][0] == info["q13"][1] == 0.3 and info["n_red"] == 1
    # all equal: q1 == q3 == threshold, nothing kept (n_red == 0: ARACNE has nothing to check)
    info, _ = _lr_case(engine, POS, (*rand_ab(50), np.full(50, 0.2)))
    assert info["n_red"] == 0 and info["n_pool"] == 0


@pytest.mark.gpu
def test_tukey_signed_zeros_and_denormals(engine):
    """Slightly negative MI values (the f64 sort key), 0.0 / -0.0, denormals at the quantiles and around the threshold."""
    rng = np.random.default_rng(4)
    L = 30
    POS = _ascending(L)
    base = np.array([-1e-17, -0.0, 0.0, 5e-324, 1e-310, 2.2250738585072014e-308, -1e-17, 0.0, -0.0, 1e-300, 3e-324, 0.5, 0.25])
    for v in (base, np.r_[base, np.full(8, -0.0)], np.r_[base[:11], 5e-324, 5e-324], np.r_[np.full(9, -1e-17), 1e-310, 0.0, 0.0]):
        v = v[rng.permutation(len(v))]
        a = rng.integers(0, L // 2, len(v))
        _lr_case(engine, POS, (a, a + rng.integers(1, L // 2, len(v)), v))


@pytest.mark.gpu
@pytest.mark.parametrize("ml_off", [0, 1, 100, -1])
def test_tukey_fallback_boundary(engine, ml_off):
    """min_links == n (fallback taken), n == min_links - 1 and min_links > n (never taken), min_links == n - 1; at n = 300 both
    fallback probabilities clamp at 0, at n = 6000 they are 1/3 and 1/6."""
    rng = np.random.default_rng(5 + ml_off)
    for n, L, how in ((300, 40, "oracle"), (6000, 400, "numpy")):
        POS = _ascending(L)
        a = rng.integers(0, L // 2, n)
        v = np.round(rng.exponential(1.0, n) * 16) / 16
        info, _ = _lr_case(engine, POS, (a, a + rng.integers(1, L // 2, n), v), min_links=n + ml_off, aracne=how)
        assert info["fallback"] == (ml_off <= 0)


@pytest.mark.gpu
def test_tukey_fallback_warning_of_the_python_layer(engine):
    rng = np.random.default_rng(6)
    L, n = 40, 300
    POS = _ascending(L)
    st, uqe, r = _meta(engine, POS)
    a = rng.integers(0, L // 2, n)
    b = a + rng.integers(1, L // 2, n)
    engine.links_import(1, a, b, np.round(rng.exponential(1.0, n) * 16) / 16)
    sd = SnpDat(states=st, POS=POS.astype(np.int32), g=float(G), uqe=uqe, r=r)
    sr = pd.DataFrame(dict(pos1=POS[[3]], pos2=POS[[1]], MI=[0.0]))
    with pytest.warns(UserWarning, match=re.escape("Not enough lr links pass the Tukey criteria, ~5000 top links were retained instead")):
        out = LR.analyse_long_range_links(engine, sd, sr, min_links=n)
    assert out["fallback"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = LR.analyse_long_range_links(engine, sd, sr, min_links=n + 1)
    assert not out["fallback"]


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [0, 1, 700])
def test_tukey_short_range_rows_below_the_threshold(engine, ns):
    """Short-range rows of the caller that all fall below the threshold add nothing to the pool (ns > n for 700)."""
    rng = np.random.default_rng(7 + ns)
    L, n = 50, 500
    POS = _ascending(L)
    a = rng.integers(0, L // 2, n)
    v = np.round(rng.exponential(1.0, n) * 16) / 16
    sa = rng.integers(0, L - 1, ns)
    sr = (sa, sa + 1, rng.uniform(-0.01, 0.01, ns))
    info, _ = _lr_case(engine, POS, (a, a + rng.integers(1, L // 2, n), v), sr=sr)
    assert info["n_pool"] == info["n_red"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [255, 256, 257])
def test_tukey_segment_edges(engine, n):
    rng = np.random.default_rng(n)
    L = 64
    POS = _ascending(L)
    a = rng.integers(0, L // 2, n)
    v = np.round(rng.exponential(1.0, n) * 16) / 16
    sa = rng.integers(0, L - 2, n)
    sr = (sa, sa + 2, np.round(rng.exponential(1.0, n) * 16) / 16)
    info, _ = _lr_case(engine, POS, (a, a + rng.integers(1, L // 2, n), v), sr=sr)
    assert info["n_red"] > 0


@pytest.mark.gpu
def test_tukey_and_ldmap_beyond_the_grid_stride(engine):
    """A table longer than 16384 x 256 rows: the grid-stride loops of k_mi_keys and the LD-map kernels go round more than once."""
    rng = np.random.default_rng(8)
    n, L = 16384 * 256 + 4099, 3000
    POS = _ascending(L, 7)
    a = rng.integers(0, L, n).astype(np.int32)
    b = ((a + rng.integers(1, L, n)) % L).astype(np.int32)
    v = np.round(rng.exponential(1.0, n) * 256) / 256
    sa = rng.integers(0, L - 1, 300_001)
    sr = (sa, sa + 1, np.round(rng.exponential(1.0, len(sa)) * 256) / 256)
    info, _ = _lr_case(engine, POS, (a, b, v), sr=sr, aracne=None)
    assert info["n_red"] > 1000
    engine.links_import(0, *sr)
    ref = orc.ld_map(dict(pos1=POS[b], pos2=POS[a], MI=v), dict(pos1=POS[sr[1]], pos2=POS[sr[0]], MI=sr[2]), reducer=11)
    htm, n_pos, r = engine.ldmap(11)
    assert n_pos == len(ref["pos_vec"]) == L and r == 11 and htm.shape == ref["htm"].shape
    np.testing.assert_allclose(htm, ref["htm"], rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------------------------------------
# GPU: ARACNE, long-range path
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_aracne_tied_triangles(engine):
    """Triangles whose MI values tie pairwise (strict < : a tie never makes a link indirect), and one value above the others."""
    rng = np.random.default_rng(9)
    L = 60
    POS = _ascending(L)
    rows = []
    for t, (mxz, mxy, mzy) in enumerate([(0.5, 0.5, 0.5), (0.5, 0.5, 0.75), (0.5, 0.75, 0.5), (0.5, 0.75, 0.75), (0.75, 0.5, 0.5),
                                         (0.5, 0.625, 0.625), (0.625, 0.625, 0.75), (0.5, 0.75, 0.75)]):
        x, y, z = 3 * t, 3 * t + 1, 3 * t + 2
        rows += [(z, x, mxz), (y, x, mxy), (y, z, mzy)]
    rows = np.array(rows)
    lr = _cat((rows[:, 0], rows[:, 1], rows[:, 2]), _filler(rng, L, 200))
    _, flags = _lr_case(engine, POS, lr)
    assert 0 < flags.sum() < len(flags)


def _hub_tables(rng, d, L, H, P1, P2, orient):
    """Hub H with spokes to d neighbours; partners P1 / P2 linked to H by a checked link of MI 0.5.  P1 shares all d neighbours with MI
    0.25 but one, the LAST in index order, at 0.75 (indirect: found only past lane 63 of the walk); P2 shares three neighbours, one of them
    at 0.5 (a tie: direct).  orient 'x': the hub on the to side (b = pos1, X), 'z': on the from side."""
    nb = np.array([i for i in range(L) if i not in (H, P1, P2)])[:d]
    assert len(nb) == d
    hub = (np.full(d, H), nb, np.full(d, 0.75))
    m1 = np.full(d, 0.25)
    m1[np.argmax(nb)] = 0.75
    p1 = (nb, np.full(d, P1), m1)
    k = min(d, 3)
    p2 = (nb[:k], np.full(k, P2), np.r_[0.5, np.full(k - 1, 0.25)])
    chk = (np.array([P1, P2]), np.array([H, H]), np.array([0.5, 0.5]))
    if orient == "z":
        chk = (chk[1], chk[0], chk[2])
    return chk, hub, p1, p2


@pytest.mark.gpu
@pytest.mark.parametrize("orient", ["x", "z"])
@pytest.mark.parametrize("d", [1, 63, 64, 65, 3000])
def test_aracne_hubs(engine, d, orient):
    rng = np.random.default_rng(d)
    L = d + 4
    POS = _ascending(L)
    H, P1, P2 = (0, L - 1, L - 2) if orient == "x" else (L - 1, 0, 1)     # SNP indices 0 and L - 1
    chk, hub, p1, p2 = _hub_tables(rng, d, L, H, P1, P2, orient)
    # spokes and partners in the long-range table (checked too), or in the caller's short-range rows (pooled only)
    for split in ("lr", "sr"):
        if split == "lr":
            lr, sr = _cat(chk, hub, p1, p2), (E32, E32, E64)
        else:
            lr, sr = chk, _cat(hub, p1, p2)
        lr = _cat(lr, _filler(rng, L, 4 * len(lr[0]) + 4 * len(sr[0]) + 50))
        info, flags = _lr_case(engine, POS, lr, sr=sr, aracne="oracle" if d < 100 else "numpy")
        red = engine.lr_reduced()
        f = dict(zip(zip(red["a"].tolist(), red["b"].tolist()), flags.tolist()))
        c1, c2 = (int(chk[0][0]), int(chk[1][0])), (int(chk[0][1]), int(chk[1][1]))
        assert f[c1] is False and f[c2] is True, (split, f[c1], f[c2])


@pytest.mark.gpu
def test_aracne_third_vertex_only_through_short_range_rows(engine):
    rng = np.random.default_rng(12)
    L = 40
    POS = _ascending(L)
    # checked links (x, z); the paths x - y - z exist only among the caller's short-range rows
    chk = (np.array([0, 5, 10, 15]), np.array([1, 6, 11, 16]), np.array([0.5, 0.5, 0.5, 0.5]))
    sr = (np.array([2, 2, 7, 7, 12, 12, 39, 39]), np.array([0, 1, 5, 6, 10, 11, 15, 16]),
          np.array([0.75, 0.75, 0.75, 0.5, 0.625, 0.875, 0.75, 0.75]))
    lr = _cat(chk, _filler(rng, L, 100))
    _, flags = _lr_case(engine, POS, lr, sr=sr)
    assert list(flags) == [False, True, False, False]


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["ascending", "permuted"])
def test_aracne_repeated_positions(engine, order):
    """Every position held by two SNPs (no pool row joins two SNPs of one position): runARACNE works on positions, so two SNPs at one
    position are one node, and a (node, neighbour) pair joined by several rows takes the MI of its first row in pool order."""
    rng = np.random.default_rng(13 if order == "ascending" else 14)
    for trial in range(4):
        L = 60
        POS = np.repeat(np.sort(rng.choice(np.arange(1, 400), L // 2, replace=False)) * 10, 2)
        if order == "permuted":
            POS = POS[rng.permutation(L)]
        lr = _random_pool(rng, POS, 200, [0.25, 0.375, 0.5, 0.625, 0.75])
        sr = _random_pool(rng, POS, 100, [0.25, 0.5, 0.75])
        lr = _cat(lr, _filler(rng, L, 1300, avoid_pos=POS))
        _lr_case(engine, POS, lr, sr=sr)


@pytest.mark.gpu
def test_aracne_random_tied_pools(engine):
    """Random pools with tied MI values at unique positions, ascending and permuted, checked by the oracle."""
    rng = np.random.default_rng(15)
    for trial in range(4):
        L = 80
        POS = np.sort(rng.choice(np.arange(1, 10_000), L, replace=False)) * 10
        if trial % 2:
            POS = POS[rng.permutation(L)]
        lr = _random_pool(rng, POS, 250, [0.25, 0.375, 0.5, 0.625, 0.75])
        sr = _random_pool(rng, POS, 120, [0.25, 0.5, 0.75])
        lr = _cat(lr, _filler(rng, L, 1500))
        _lr_case(engine, POS, lr, sr=sr)


# ------------------------------------------------------------------------------------------------------------------------------
# GPU: ARACNE, short-range path
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_aracne_short_range_path_with_ties_and_a_hub(engine):
    """merge_n_sort_sr_links_device(..., run_aracne=True) on an imported short-range table with planted MI ties and a hub, against the
    oracle's mergeNsort_sr_links + runARACNE on the same table (unique positions)."""
    rng = np.random.default_rng(16)
    L, sr_dist = 300, 20000.0
    POS = np.arange(L) + 1              # every length 1..L-1 occurs many times (mean_dist is looked up by the value of len)
    paint = rng.integers(1, 4, L).astype(np.int32)
    a, b = np.triu_indices(L, 1)
    ln = np.abs(POS[b] - POS[a]).astype(float)
    keep = (ln < sr_dist) & (rng.random(len(a)) < 0.3)
    hub = L // 2
    keep |= ((a == hub) | (b == hub)) & (ln < sr_dist)                       # the hub keeps every partner in range
    a, b, ln = a[keep], b[keep], ln[keep]
    mi = 0.05 * (ln + 1) ** -0.3 + rng.exponential(0.02, len(a))
    mi = np.round(mi * 512) / 512                                             # ties everywhere
    mi[(a == hub) | (b == hub)] = np.round(mi[(a == hub) | (b == hub)] * 1.6 * 64) / 64
    _meta(engine, POS)
    engine.set_snp_meta(_ALN[L][2], _ALN[L][1], POS.astype(np.int32), paint, float(G))
    engine.links_import(0, a.astype(np.int32), b.astype(np.int32), mi)
    engine.links_import(1, E32, E32, E64)
    tab = dict(pos1=POS[b].astype(float), pos2=POS[a].astype(float), clust1=paint[b], clust2=paint[a], len=ln, MI=mi)
    by_clust = [{k: v[(tab["clust1"] == ci) | (tab["clust2"] == ci)] for k, v in tab.items()} for ci in (1, 2, 3)]
    # a cut-off in a wide gap of the oracle's srp_max: the two beta optimisers agree to ~1e-6, far inside it
    probe, _ = orc.merge_n_sort_sr_links(by_clust, 3, sr_dist, -1e300)
    s = np.sort(np.asarray(probe["srp_max"]))
    s = s[int(0.6 * len(s)): int(0.9 * len(s))]
    gi = int(np.argmax(np.diff(s)))
    assert s[gi + 1] - s[gi] > 1e-4
    cut = 0.5 * (s[gi] + s[gi + 1])
    ored, ochk = orc.merge_n_sort_sr_links(by_clust, 3, sr_dist, cut)
    oflags = orc.run_aracne(ored["pos1"], ored["pos2"], ored["MI"], ochk["pos1"], ochk["pos2"], ochk["MI"])
    red, flags, aux = SRP.merge_n_sort_sr_links_device(engine, 3, sr_dist, cut, POS, paint, float(G), run_aracne=True)
    pos1, pos2 = POS[red["b"]], POS[red["a"]]
    assert len(pos1) == len(ored["MI"]) > 50
    assert np.array_equal(pos1, np.asarray(ored["pos1"])) and np.array_equal(pos2, np.asarray(ored["pos2"]))
    assert np.array_equal(red["MI"], np.asarray(ored["MI"]))
    assert np.array_equal(flags, oflags)
    assert 0 < flags.sum() < len(flags)


# ------------------------------------------------------------------------------------------------------------------------------
# GPU: LD map
# ------------------------------------------------------------------------------------------------------------------------------
def _ldmap_case(engine, POS, lr, sr, reducer=0, win=None):
    """Device LD map against orc.ld_map; when the oracle refuses, the device must refuse too."""
    POS = np.asarray(POS, dtype=np.int64)
    _meta(engine, POS)
    lr = tuple(np.asarray(x) for x in lr)
    sr = tuple(np.asarray(x) for x in sr)
    engine.links_import(1, lr[0].astype(np.int32), lr[1].astype(np.int32), lr[2].astype(np.float64))
    engine.links_import(0, sr[0].astype(np.int32), sr[1].astype(np.int32), sr[2].astype(np.float64))
    d = lambda t: dict(pos1=POS[t[1].astype(np.int64)], pos2=POS[t[0].astype(np.int64)], MI=t[2].astype(np.float64))
    try:
        with np.errstate(invalid="ignore", divide="ignore"):
            ref = orc.ld_map(d(lr), d(sr), reducer=reducer or None, from_=win[0] if win else None, to=win[1] if win else None)
    except ValueError:
        with pytest.raises(RuntimeError):
            engine.ldmap(reducer, *(win or (0, 0)))
        return None
    htm, n_pos, r = engine.ldmap(reducer, *(win or (0, 0)))
    assert n_pos == len(ref["pos_vec"]) and r == ref["reducer"] and htm.shape == ref["htm"].shape
    np.testing.assert_allclose(htm, ref["htm"], rtol=0, atol=1e-12, equal_nan=True)
    assert np.array_equal(htm, htm.T, equal_nan=True)
    return htm, n_pos, r


def _chain(rng, L, extra):
    """Links touching every SNP (a chain) plus random ones, MI with ties."""
    a = np.r_[np.arange(L - 1), rng.integers(0, L, extra)]
    b = np.r_[np.arange(1, L), rng.integers(0, L, extra)]
    ok = a != b
    return a[ok], b[ok], np.round(rng.exponential(0.2, ok.sum()) * 64) / 64


@pytest.mark.gpu
def test_ldmap_block_geometry(engine):
    rng = np.random.default_rng(20)
    L = 100
    POS = _ascending(L, 37)
    lr, sr = _chain(rng, L, 300), _chain(rng, L, 50)
    assert _ldmap_case(engine, POS, lr, sr, reducer=7)[0].shape == (14, 14)       # n_pos % r != 0: ranks 98, 99 fall outside
    htm, _, _ = _ldmap_case(engine, POS, lr, sr, reducer=100)                      # r == n_pos: B == 1, 0 / 0 -> NaN on both sides
    assert htm.shape == (1, 1) and np.isnan(htm).all()
    _ldmap_case(engine, POS, lr, (E32, E32, E64), reducer=9)                       # long-range only
    _ldmap_case(engine, POS, (E32, E32, E64), sr, reducer=9)                       # short-range only
    # links inside one block (the diagonal gets both i, j and j, i) next to links across blocks
    inb = (np.array([0, 10, 11, 30]), np.array([3, 14, 13, 31]), np.array([0.5, 0.25, 0.125, 1.0]))
    _ldmap_case(engine, POS, _cat(inb, _chain(rng, L, 0)), (E32, E32, E64), reducer=5)
    # many links summed into one cell
    many = (rng.integers(0, 5, 5000), rng.integers(5, 10, 5000), rng.uniform(0, 1, 5000))
    htm, _, _ = _ldmap_case(engine, POS, _cat(many, _chain(rng, L, 0)), sr, reducer=10)
    assert htm[0, 0] == 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("n_pos,r_want", [(1499, None), (2500, 2), (3500, 4)])
def test_ldmap_default_reducer_rounding(engine, n_pos, r_want):
    """reducer = round(n_pos / 1000), half to even: 1499 -> 1 (the unreduced branch, refused), 2500 -> 2, 3500 -> 4."""
    rng = np.random.default_rng(n_pos)
    POS = _ascending(n_pos, 11)
    out = _ldmap_case(engine, POS, _chain(rng, n_pos, 2000), _chain(rng, n_pos, 500))
    assert (out is None) == (r_want is None)
    if out is not None:
        assert out[1] == n_pos and out[2] == r_want


@pytest.mark.gpu
def test_ldmap_windows(engine):
    rng = np.random.default_rng(21)
    L = 120
    POS = _ascending(L, 100)
    lr, sr = _chain(rng, L, 400), _chain(rng, L, 100)
    # window edges ON link positions: those positions are outside pos_vec (from < pos < to), their links have no level
    out = _ldmap_case(engine, POS, lr, sr, reducer=4, win=(int(POS[10]), int(POS[90])))
    assert out[1] == 79
    _ldmap_case(engine, POS, lr, sr, reducer=3, win=(int(POS[0]), int(POS[L - 1])))
    _ldmap_case(engine, POS, lr, sr, reducer=3, win=(int(POS[10]) - 1, int(POS[90]) + 1))
    # no position inside the window: both sides refuse, with an explicit and with the default reducer
    for red in (2, 0):
        assert _ldmap_case(engine, POS, lr, sr, reducer=red, win=(int(POS[20]) + 1, int(POS[21]) - 1)) is None
        with pytest.raises(RuntimeError):
            engine.ldmap(red, int(POS[20]) + 1, int(POS[21]) - 1)


@pytest.mark.gpu
def test_ldmap_rescale_is_a_division(engine):
    """.rescale01 divides by max - min (R/LDSummaryPlot.R:157-163): the largest cell is exactly 1.  One link per cell (no order of atomics to
    depend on) and a largest MI for which a product with 1 / (max - min) rounds to 1 - 2^-53."""
    L = 40
    POS = _ascending(L, 10)
    lo = np.log10(1e-5)
    top = next(v for v in 0.25 + np.arange(1, 4096) / 4096
               if (np.log10((v + v) / 4 + 1e-5) - lo) * (1.0 / (np.log10((v + v) / 4 + 1e-5) - lo)) != 1.0)
    a = np.arange(0, L, 2)
    mi = np.r_[np.linspace(0.01, 0.2, len(a) - 1), top]
    htm, _, _ = _ldmap_case(engine, POS, (a, a + 1, mi), (E32, E32, E64), reducer=2)
    assert htm.shape == (20, 20) and htm[19, 19] == 1.0 and htm.max() == 1.0 and htm.min() == 0.0
