"""CPU: the host rules behind ``background.apc_links`` (include/ldweaver_amd.h 22) — ``pick_threshold`` against the plain-loop statement of
tests/scoresel_ref.py on hand-made histograms, the weights of the average product correction from hand-made backgrounds, the exports and ABI names, the
score of csrc/ldw_score.h compiled for the host against numpy on values that tell a fused evaluation from an unfused one, and the planted example through
the C oracle alone: selected by the corrected score over every pair it comes first, selected by raw MI it is not among the top 700.  No GPU call."""
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import c_oracle
import decay_ref as D
import ldw_oracle as orc
import ldweaver_amd
import scoresel_ref as S
import snpsum_ref as R
from ldweaver_amd import _lib as L
from ldweaver_amd import background as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hist_of(counts):
    h = np.zeros(S.NBINS, dtype=np.uint64)
    for k, v in counts.items():
        h[k] = v
    return h


EDGE = lambda Bk: float(D.bucket_lo(Bk))

HISTS = {
    "edge": (hist_of({0: 50, 100: 7, 2000: 3, 3000: 4, 4095: 1}), 8),           # cum(2000) == 8 exactly: the bucket's lower edge, cap == top
    "inside": (hist_of({0: 50, 100: 7, 2000: 3, 3000: 4, 4095: 1}), 6),         # rank 6 lies inside bucket 2000: the whole bucket comes along, cap 8
    "never": (hist_of({0: 1000, 5: 2, 9: 1}), 10),                              # fewer than top above bucket 0: B* = 1, cap 3
    "empty": (hist_of({}), 5),                                                  # B* = 1, cap 0
    "top_bucket": (hist_of({4095: 12}), 5),                                     # everything in the last bucket
    "bucket_one": (hist_of({0: 9, 1: 4}), 4),
    "huge": (hist_of({0: 1 << 62, 7: (1 << 63) + 5, 8: 1 << 63}), 1 << 63),     # counts whose sum passes 2^64
}
EXPECT = {"edge": (EDGE(2000), 8), "inside": (EDGE(2000), 8), "never": (EDGE(1), 3), "empty": (EDGE(1), 0), "top_bucket": (EDGE(4095), 12),
          "bucket_one": (EDGE(1), 4), "huge": (EDGE(8), 1 << 63)}


@pytest.mark.parametrize("case", sorted(HISTS))
def test_pick_threshold_on_hand_made_histograms(case):
    hist, top = HISTS[case]
    thr, cap = B.pick_threshold(hist, top)
    assert (thr, cap) == S.pick_threshold(hist, top) == EXPECT[case]
    assert isinstance(cap, int) and isinstance(thr, float) and thr >= 2.0 ** -20
    # the edge is the smallest value of its bucket: the double below it falls in the bucket below, and cap counts the buckets from it on
    Bk = int(D.mi_bucket(np.array([thr]))[0])
    assert Bk >= 1 and int(D.mi_bucket(np.array([D.below(thr)]))[0]) == Bk - 1
    assert cap == sum(int(x) for x in hist[Bk:])


def test_pick_threshold_bits_and_shape():
    thr, cap = B.pick_threshold(hist_of({1234: 3}), 1)
    assert np.array([thr]).view(np.int64)[0] == (1234 + ((1023 - 20) << 7)) << 45 and cap == 3
    assert B.pick_threshold(hist_of({1234: 3}), 4) == (EDGE(1), 3)              # never reached
    with pytest.raises(ValueError):
        B.pick_threshold(np.zeros(100, dtype=np.uint64), 1)


def background_of(n, sumq):
    n, sumq = np.asarray(n, dtype=np.int64), np.asarray(sumq, dtype=np.int64)
    k = n.shape[1]
    return B.SnpBackground(n, sumq, np.full((2, k), np.nan), np.zeros((2, k), np.int64), n.sum(axis=1) // 2, 10 * np.arange(1, k + 1), 1000.0, 15.0, (np.inf, np.inf))


def test_weights_with_a_snp_without_pairs_and_sums_past_2_61():
    one = 1 << 40
    bg = background_of([[2, 0, 2, 0], [4, 4, 0, 0]], [[one, 0, 3 * one, 0], [2 * one, one, 0, 0]])
    w = B.apc_weights(bg, "lr")
    overall = (3 * one) / 8 / 2.0 ** 40
    assert np.array_equal(w, np.array([0.5, 0.25, 0.0, 0.0]) / np.sqrt(overall)) and w[2] == 0.0 and w[3] == 0.0      # n = 0: the mean is NaN, the weight 0
    assert np.isnan(bg.mean("lr")[2]) and np.isfinite(w).all()
    wa = B.apc_weights(bg, "all")
    assert np.array_equal(wa, np.array([0.5, 0.25, 1.5, 0.0]) / np.sqrt(7 / 12)) and wa[3] == 0.0
    big = 1 << 61                                                              # six sums of 2^61 pass 2^63: the overall mean is taken in Python's integers
    bg2 = background_of(np.full((2, 6), 4), np.stack([np.full(6, big), np.array([big, big - 3, big, 5, big, big])]))
    assert int(bg2.sumq[0].sum()) < 0
    w2 = B.apc_weights(bg2, "sr")
    assert np.array_equal(w2, np.full(6, 2.0 ** 19 / np.sqrt(2.0 ** 19))) and (np.abs(w2 * w2 - 2.0 ** 19) <= 2.0 ** -33).all()      # (sqrt and product round: 2 ulp)
    w3 = B.apc_weights(bg2, "lr")
    assert w3[3] == (5 / 4 / 2.0 ** 40) / np.sqrt((5 * big + 2) / 24 / 2.0 ** 40) and (w3 > 0).all()


def test_an_overall_mean_that_is_not_positive_raises():
    zero = background_of([[2, 2], [2, 2]], [[0, 0], [0, 0]])
    with pytest.raises(ValueError, match="overall mean"):
        B.apc_weights(zero, "lr")
    negative = background_of([[2, 2], [2, 2]], [[0, 0], [-5, -7]])
    with pytest.raises(ValueError, match="overall mean"):
        B.apc_weights(negative, "lr")
    nothing = background_of([[0, 0], [0, 0]], [[0, 0], [0, 0]])               # no pair at all: NaN
    with pytest.raises(ValueError, match="overall mean"):
        B.apc_weights(nothing, "all")
    with pytest.raises(ValueError):
        B.apc_weights(zero, "long")


def test_exports():
    for name in ("apc_links", "pick_threshold"):
        assert name in ldweaver_amd.__all__ and getattr(ldweaver_amd, name) is getattr(B, name)
    from ldweaver_amd.engine import Engine
    for name in ("mi_score_scan", "mi_score_links", "score_select_report", "debug_score_scan", "debug_score_links"):
        assert callable(getattr(Engine, name))
    api = {"ldw_mi_score_scan", "ldw_mi_score_links"}
    debug = {"ldw_debug_score_scan", "ldw_debug_score_links", "ldw_score_select_report"}
    assert api <= set(L.declared_symbols("ldweaver_amd.h")) and debug <= set(L.declared_symbols("ldweaver_amd_debug.h"))
    for name in api | debug:
        assert hasattr(L.lib(), name)
    assert B.CLS_MASK == {"sr": 1, "lr": 2, "all": 3}


def fused(mi, wa, wb):
    """mi - wa wb rounded once, as a fused multiply-add would: exact rationals, then the nearest double."""
    x = Fraction(float(mi)) - Fraction(float(wa)) * Fraction(float(wb))
    return float(x)                                                             # (Fraction -> float rounds to nearest, ties to even)


def score_values():
    """Triples whose product is inexact, so that one rounding differs from two, besides signed zeros, infinities and NaN."""
    rng = np.random.default_rng(33)
    wa, wb = rng.uniform(0.1, 1.0, 4000), rng.uniform(0.1, 1.0, 4000)
    mi = wa * wb * (1 + rng.integers(-3, 4, 4000) * 2.0 ** -52)                 # the difference is a few units of the product's last place
    sp = np.array([[0.0, 0.0, 0.0], [-0.0, 0.0, 5.0], [0.25, 0.5, 0.5], [0.25, -0.5, 0.5], [np.nan, 1.0, 1.0], [np.inf, 1e200, 1e200], [1.0, 1e200, 1e200],
                   [5e-324, 1e-200, 1e-200], [0.1, 0.3, 1.0 / 3.0], [1e-300, 1e-160, 1e-160]])
    return np.concatenate([np.stack([mi, wa, wb], axis=1), sp])


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_the_score_of_the_header_on_the_host_is_not_fused(tmp_path):
    v = score_values()
    ref = S.score(v[:, 0], v[:, 1], v[:, 2])
    one = np.array([fused(*t) if np.isfinite(t).all() and abs(t[1] * t[2]) < 1e300 else np.nan for t in v[:4000]])
    assert (one != ref[:4000]).sum() > 1000                                     # the values do tell the two evaluations apart
    with open("/proc/cpuinfo") as f:
        has_fma = " fma " in f.read()
    text = "".join("%016x %016x %016x\n" % tuple(int(x) for x in np.array(t).view(np.uint64)) for t in v)
    for flags in (["-O1"], ["-O3", "-ffp-contract=fast"] + (["-mfma"] if has_fma else [])):      # the header, not the command line, keeps the product apart
        exe = str(tmp_path / ("score_check" + str(len(flags))))
        subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "host", "score_check.cpp")], check=True, timeout=300)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        got = np.array([int(line, 16) for line in out.stdout.split()], dtype=np.uint64).view(np.float64)
        assert got.shape == ref.shape and S.same_bits(got, ref), (flags, np.flatnonzero(got.view(np.int64) != ref.view(np.int64))[:5])
    assert np.signbit(ref[4001]) and ref[4002] == 0.0 and np.isnan(ref[4004]) and np.isnan(ref[4005]) and ref[4006] == -np.inf


def test_the_statement_equals_a_double_loop():
    rng = np.random.default_rng(5)
    nf, nt, g = 7, 9, 1000.0
    pf, pt = rng.integers(1, 1001, nf), rng.integers(1, 1001, nt)
    mi = np.exp(rng.uniform(-16, 0, (nf, nt)))
    mi[2, 3], mi[4, 4], mi[0, 8] = np.nan, 0.0, -0.0
    wf, wt = rng.uniform(-0.3, 0.3, nf), rng.uniform(-0.3, 0.3, nt)
    idf, idt = rng.permutation(100)[:nf], rng.permutation(100)[:nt] + 100
    for mask in (1, 2, 3):
        for sr in (0.0, 150.0, np.inf):
            sc = S.scan(mi, pf, pt, g, False, sr, mask, wf, wt)
            lk, prf, prt = S.links(mi, pf, pt, g, False, sr, mask, idf, idt, wf, wt, 0.01, sc["best_f"], sc["best_t"])
            hist, npairs, nan, listed = np.zeros(S.NBINS, np.uint64), 0, 0, set()
            bf, bt = [None] * nf, [None] * nt
            for a in range(nf):
                for b in range(nt):
                    d = (float(pt[b]) - float(pf[a])) % g
                    cls = 1 if 0.5 * g - abs(d - 0.5 * g) <= sr else 2
                    if a == b or not cls & mask:
                        continue
                    npairs += 1
                    s = float(mi[a, b]) - float(wf[a]) * float(wt[b])
                    if s != s:
                        nan += 1
                        continue
                    hist[int(D.mi_bucket(np.array([s]))[0])] += 1
                    k = int(R.f64_key(np.array([s]))[0])
                    if bf[a] is None or k > bf[a][0] or (k == bf[a][0] and idt[b] < bf[a][2]):
                        bf[a] = (k, s, int(idt[b]))
                    if bt[b] is None or k > bt[b][0] or (k == bt[b][0] and idf[a] < bt[b][2]):
                        bt[b] = (k, s, int(idf[a]))
                    if s >= 0.01:
                        listed.add((int(idf[a]), int(idt[b])))
            assert np.array_equal(sc["hist"], hist) and sc["npairs"] == npairs and sc["nan"] == nan
            assert S.same_bits(sc["best_f"], [np.nan if x is None else x[1] for x in bf]) and S.same_bits(sc["best_t"], [np.nan if x is None else x[1] for x in bt])
            assert {(a, b) for a, b, _, _ in lk} == listed
            assert prf.tolist() == [-1 if x is None else x[2] for x in bf] and prt.tolist() == [-1 if x is None else x[2] for x in bt]


def test_the_planted_example_through_the_c_oracle():
    """Forty lineage markers and one planted pair (tests/snpsum_ref.planted_apc).  The statement of (22) applied to the C oracle's MI with the weights of the
    average product correction: the top 10 by score start with the planted pair, which a selection of the top 700 by raw MI does not contain (it is rank 781
    there: all 780 marker pairs rank above it, tests/test_background_host.py)."""
    st, pos, g, sr, markers, (pa, pb) = R.planted_apc()
    uqe, r = orc.uqe_r(st)
    idx = np.arange(len(st))
    M = c_oracle.mi_block(st, np.ones(st.shape[1]), r, uqe, idx, idx)
    rows, cols, npairs, _ = R.snp_summary(M, pos, pos, g, True, sr, (np.inf, np.inf))
    tot = R.empty_total(len(st))
    R.fold(tot, rows, idx)
    R.fold(tot, cols, idx)
    bg = B.SnpBackground(tot["n"], tot["sumq"], tot["max"], tot["nge"], npairs, pos, g, sr, (np.inf, np.inf))
    w = B.apc_weights(bg, "lr")
    sc = S.scan(M, pos, pos, g, True, sr, 2, w, w)
    assert sc["npairs"] == 7140 == int(sc["hist"].sum()) and sc["nan"] == 0
    thr, cap = B.pick_threshold(sc["hist"], 10)
    assert (thr, cap) == S.pick_threshold(sc["hist"], 10) and cap >= 10
    lk, prf, prt = S.links(M, pos, pos, g, True, sr, 2, idx, idx, w, w, thr, sc["best_f"], sc["best_t"])
    assert len(lk) == cap                                                       # bucket edges are monotone in the value
    top = sorted(lk, key=lambda t: (-np.array([t[3]], dtype=np.int64).view(np.float64)[0], t[0], t[1]))[:10]
    assert (top[0][0], top[0][1]) == (max(pa, pb), min(pa, pb))
    s0, s1 = (np.array([t[3]], dtype=np.int64).view(np.float64)[0] for t in top[:2])
    print("planted score", s0, "runner-up", s1, "thr", thr, "cap", cap)
    assert s1 < 0.5 * s0
    a, b = np.tril_indices(len(st), -1)
    raw = M[a, b]
    order = np.argsort(-raw, kind="stable")
    p = int(np.flatnonzero((a == max(pa, pb)) & (b == min(pa, pb)))[0])
    rank = int(np.flatnonzero(order == p)[0]) + 1
    assert rank == 781 and p not in set(order[:700].tolist())
    tot2 = S.empty_total(len(st))                                              # each of the two is the other's best partner: the two sides folded per SNP
    S.fold(tot2, sc, idx, idx)
    lk2, pf2, pt2 = S.links(M, pos, pos, g, True, sr, 2, idx, idx, w, w, thr, tot2["best"], tot2["best"])
    part = np.full(len(st), -1, dtype=np.int64)
    S.fold_partner(part, pf2, idx)
    S.fold_partner(part, pt2, idx)
    assert part[pa] == pb and part[pb] == pa and lk2 == lk
