"""CPU: the LD-decay statement (tests/decay_ref.py) against a double loop, the host rules of ldweaver_amd/decay.py against it and against the values
themselves, the exports, and the planted example through the oracle alone.  No GPU call."""
import math
import warnings

import numpy as np
import pytest

import decay_ref as R
import ldw_oracle as orc
import ldweaver_amd
from ldweaver_amd import _lib as L
from ldweaver_amd import decay as D


def loop_hist(mi, pos_f, pos_t, g, diag, cuts, mi_shift):
    """The statement pair by pair, with Python's own arithmetic and struct for the bits."""
    import struct
    nf, nt = mi.shape
    nb = 4096 >> mi_shift
    hist = np.zeros((len(cuts) + 1, nb), dtype=np.uint64)
    mx = [None] * (len(cuts) + 1)
    n = 0
    for a in range(nf):
        for b in range(nt):
            if (a <= b) if diag else (a == b):
                continue
            d = (float(pos_t[b]) - float(pos_f[a])) % g
            ln = 0.5 * g - abs(d - 0.5 * g)
            k = sum(1 for c in cuts if c < ln)
            v = float(mi[a, b])
            u = struct.unpack("<q", struct.pack("<d", v))[0]
            bk = 0 if u <= 0 else min(max((u >> 45) - ((1023 - 20) << 7), 0), 4095)
            hist[k, bk >> mi_shift] += np.uint64(1)
            mx[k] = v if mx[k] is None else max(mx[k], v)
            n += 1
    return hist, np.array([np.nan if m is None else m for m in mx]), n


@pytest.mark.parametrize("nf,nt,diag,shift", [(1, 1, False, 0), (1, 2, False, 3), (2, 1, False, 6), (7, 5, False, 3), (6, 6, True, 0), (1, 1, True, 3), (9, 9, False, 6)])
def test_the_numpy_statement_equals_a_double_loop(nf, nt, diag, shift):
    rng = np.random.default_rng(nf * 100 + nt)
    g = 1000.0
    pos_f = rng.integers(1, 1001, nf)
    pos_t = pos_f if diag else rng.integers(1, 1001, nt)
    mi = np.where(rng.random((nf, nt)) < 0.2, -rng.random((nf, nt)), np.exp(rng.uniform(-16, 2, (nf, nt))))
    mi[0, 0] = 0.0
    cuts = [0.0, 10.0, 250.0, 499.0, 500.0, 700.0]
    h, m, n = R.profile_hist(mi, pos_f, pos_t, g, diag, cuts, shift)
    h2, m2, n2 = loop_hist(mi, pos_f, pos_t, g, diag, cuts, shift)
    assert n == n2 == (nf * (nf - 1) // 2 if diag else nf * nt - min(nf, nt)) == int(h.sum())
    assert np.array_equal(h, h2) and R.same_max(m, m2)


def test_mi_bucket_edges():
    for B in (1, 2, 8, 64, 2048, 4095):
        lo = R.bucket_lo(B)
        assert R.mi_bucket(lo) == B and R.mi_bucket(R.below(lo)) == B - 1
        assert D.bucket_lo(B) == lo
    assert R.bucket_lo(1) == 2.0 ** -20 * (1 + 1 / 128) and R.bucket_lo(4096) == 4096.0
    assert list(R.mi_bucket(np.array([0.0, -0.0, -1.0, 2.0 ** -20, 2.0 ** -21, 5000.0, 3.0]))) == [0, 0, 0, 0, 0, 4095, (21 << 7) + 64]


@pytest.mark.parametrize("shift", (0, 3, 6))
def test_the_quantile_rule_brackets_the_order_statistic(shift):
    rng = np.random.default_rng(shift)
    nb = 4096 >> shift
    for trial in range(20):
        n = int(rng.integers(1, 400))
        v = np.exp(rng.uniform(-15, 3, n)) * (rng.random(n) > 0.1)       # some exact zeros
        cuts = np.array([10.0])
        hist = np.zeros((2, nb), dtype=np.uint64)
        hist[1] = np.bincount(R.mi_bucket(v) >> shift, minlength=nb)       # bin 0 stays empty
        dec = D.LDDecay(hist, np.array([np.nan, v.max()]), cuts, 100.0, shift, n)
        for q in (0.0, 0.01, 0.5, 0.95, 0.99, 1.0, float(rng.random())):
            lo, hi = dec.quantile(q)
            rlo, rhi = R.quantile(hist, shift, q)
            assert np.array_equal(lo, rlo, equal_nan=True) and np.array_equal(hi, rhi, equal_nan=True)
            assert np.isnan(lo[0]) and np.isnan(hi[0])
            stat = np.sort(v)[min(max(math.ceil(q * n), 1), n) - 1]
            assert lo[1] <= stat < hi[1], (q, n, stat, lo[1], hi[1])
        me = dec.mean_estimate()
        assert np.isnan(me[0]) and me[1] >= 0
        width = 2.0 ** ((1 << shift) / 128)
        big = v[v >= 2.0 ** -20]
        if len(big) == n:                                                  # every value in a proper bucket: the estimate is within a bucket's width
            assert v.mean() / width <= me[1] <= v.mean() * width


def test_default_cuts():
    c = D.default_cuts(5e6)
    assert len(c) == 47 and c[0] == 100 and c[-1] < 2.5e6 and np.all(np.diff(c) > 0) and np.array_equal(c, np.rint(c))
    ratio = c[1:] / c[:-1]
    assert ratio.max() / ratio.min() < 1.05                                # geometric up to the rounding
    s = D.default_cuts(300.0, 48)                                          # 100 .. 150: duplicates removed
    assert len(s) < 47 and s[0] == 100 and s[-1] < 150 and np.all(np.diff(s) > 0)
    assert len(D.default_cuts(200.0)) == 0 and len(D.default_cuts(150.0)) == 0
    assert len(D.default_cuts(1e6, 10)) == 9


def test_exports():
    for name in ("ld_decay", "LDDecay", "default_cuts"):
        assert name in ldweaver_amd.__all__ and getattr(ldweaver_amd, name) is getattr(D, name)
    from ldweaver_amd import plots
    assert callable(plots.ld_decay_plot)
    for name in ("ldw_mi_profile", "ldw_debug_profile_hist"):
        assert name in L.declared_symbols() and hasattr(L.lib(), name)
    assert "ldw_mi_profile" in L.declared_symbols("ldweaver_amd.h") and "ldw_debug_profile_hist" in L.declared_symbols("ldweaver_amd_debug.h")


def test_background_and_suggestion_rules():
    nb = 4096 >> 3
    cuts = np.array([100.0, 200.0, 300.0, 1000.0])
    hist = np.zeros((5, nb), dtype=np.uint64)
    hi_bin, lo_bin = (int(b) >> 3 for b in R.mi_bucket(np.array([0.4, 0.01])))
    hist[0, hi_bin] = hist[1, hi_bin] = 1000
    hist[2, hi_bin] = 50                                                   # too few pairs to count
    hist[2, lo_bin] = 10
    hist[3, lo_bin] = hist[4, lo_bin] = 5000
    dec = D.LDDecay(hist, np.zeros(5), cuts, 4000.0, 3, int(hist.sum()))
    lo, hi = D.bin_edges(3)
    assert dec.background(0.95) == (lo[lo_bin], hi[lo_bin])               # bins from g / 4 = 1000 on: the last one
    assert dec.background(0.95, from_len=300.0) == (lo[lo_bin], hi[lo_bin])
    assert dec.suggest_sr_dist() == 200.0
    assert dec.suggest_sr_dist(min_pairs=10) == 300.0
    with pytest.raises(ValueError):
        dec.background(0.95, from_len=1500.0)
    flat = D.LDDecay(np.tile(hist[3], (5, 1)), np.zeros(5), cuts, 4000.0, 3, 25000)
    assert flat.suggest_sr_dist() == 0.0
    hist2 = hist.copy()
    hist2[4] = 0
    hist2[4, hi_bin] = 1000
    hist2[3, lo_bin] = 5000
    far = D.LDDecay(hist2, np.zeros(5), cuts, 4000.0, 3, int(hist2.sum()))
    with pytest.warns(RuntimeWarning):
        assert far.suggest_sr_dist(from_len=300.0, q=0.5) is None          # the background (bins 3 and 4 pooled) sits in the low bin; bin 4 itself stands out
    fr = dec.frame()
    assert list(fr.columns) == ["len_lo", "len_hi", "n_pairs", "q50", "q95", "q99", "max", "mean_est"]
    assert list(fr["len_lo"]) == [0, 100, 200, 300, 1000] and list(fr["len_hi"]) == [100, 200, 300, 1000, 2000]
    assert list(fr["n_pairs"]) == [1000, 1000, 60, 5000, 5000]


def test_the_planted_example_through_the_oracle():
    """Eight-SNP groups in tight LD, 100 bp apart, on a background of independent groups: the 0.95-quantile stands 40-fold above the background up to
    700 bp (the largest distance inside a group) and not beyond, so the suggestion is 700 for every factor between 1.5 and 30."""
    st, pos, g, cuts = R.planted_alignment()
    uqe, r = orc.uqe_r(st)
    idx = np.arange(len(st))
    M = orc.mi_block_faithful(st, np.ones(st.shape[1]), r, uqe, idx, idx)
    hist, mx, n = R.profile_hist(M, pos, pos, g, True, cuts, 3)
    assert n == 400 * 399 // 2
    dec = D.LDDecay(hist, mx, cuts, g, 3, n)
    qlo, _ = dec.quantile(0.95)
    bg = dec.background(0.95, from_len=20000)
    print("q95 lo:", qlo, "background:", bg)
    assert np.isnan(qlo[-1]) and dec.bin_pairs[-1] == 0                   # no pair lies beyond 40 000: the largest len is 39 900
    assert 0.39 <= qlo[:7].min() and qlo[:7].max() <= 0.44 and qlo[7:-1].max() <= 0.0098 and bg[0] == 0.009765625
    assert qlo[:7].min() > 30 * bg[0] and qlo[7:-1].max() <= 1.5 * bg[0]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for factor in (1.5, 2.0, 5.0, 10.0, 30.0):
            assert dec.suggest_sr_dist(0.95, factor, from_len=20000) == 700.0
