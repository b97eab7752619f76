"""The long-range selection (csrc/ldw_mi_select.inc; dispatched from select_rows and finish_span in csrc/ldw_mi_items.inc) at its structural
edges.  The reference isolates the selection from the MI arithmetic: per block the dense DEVICE MI (``engine.mi_block``) goes through the
oracle's rule in numpy — ``orc.block_pair_index`` order, the short/long split, prob as in lr_prob, ``orc.quantile7``, ``>=`` — and the pass must
reproduce n_lr_total, n_lr_kept, disc_thresh, the kept (a, b) sequence and the MI bits with ``==``: no tolerance anywhere in this file.

Every case runs cold (``reset_speculation``) and then warm, with ``set_select(0)`` (sort-free where it applies) and ``set_select(1)`` (two radix
sorts), and proves on the device MI that it reached the branch it was built for; a construction that lacks its property FAILS, it never skips.

The constants the cases sit on, restated as plain numbers (a change there: revisit the case):
  SEL_LIST = 6144          ldw_mi_select.inc: keys of the threshold's bucket k_sel_thresh keeps in LDS
  SEL_MAX = 1 << 20        ldw_mi_select.inc: candidates the sort-free path takes
  SEL_CHUNK_BITS = 1024, SEL_SUPER = 64   ldw_mi_select.inc: the three-level rank of k_sel_scatter
  NBINS = 4096             ldw_internal.h: buckets of the level-1 histogram; mi_bucket (ldw_epi.h) is restated in ``_bucket``
  margin 10                ldw_mi_items.inc, update_guess: the guess a block leaves while fewer than three thresholds of its kind are known
  0.007                    ldw_mi_items.inc, speculation_pays: blocks speculate when lr_retain_links < 0.007 lr_links_approx
  2048, square             ldw_pass_plan.h, span_candidate: what a block must be to join a span

Not reachable through the public surface (see the cases): span segments of different nt and a span segment that keeps no row (span_candidate
takes square blocks of at least 2048 SNPs without one short-range pair, and `>=` keeps the maximum of every non-empty block); the guess of a
block is not reported, so the exact-guess case brackets it with ``spec_misses`` instead.  Blocks of more than 2^28 pairs (key spaces above
2^29 bits, SEL_MAX_SUPER) are accepted up to nf * nt < 2^31 (prep_block): the last case."""
import math

import numpy as np
import pytest

import ldw_oracle as orc
from ldweaver_amd import _lib as L

pytestmark = pytest.mark.gpu

SEL_LIST = 6144
SEL_MAX = 1 << 20
NBINS = 4096
GUESS_MARGIN = 10
STEP, SR = 1000, 500.0      # SNPs 1000 apart, sr_dist below that: every off-diagonal pair is long-range


# ------------------------------------------------------------------------------------------------
# restatements of the library's integer rules
# ------------------------------------------------------------------------------------------------
def _bucket(v):
    """mi_bucket of ldw_epi.h: 128 buckets per octave from 2^-20 up, from the IEEE-754 bits; non-positive values in bucket 0."""
    u = np.ascontiguousarray(v, dtype=np.float64).view(np.int64)
    b = np.clip((u >> 45) - ((1023 - 20) << 7), 0, NBINS - 1)
    return np.where(u <= 0, 0, b)


def _ranks(n, retain, approx):
    """(prob, index, lo, hi) of quantile type 7 as lr_prob / q7_index round them (every operation on its own)."""
    prob = max(0.0, 1.0 - ((retain * (n / approx)) / n))
    index = 1.0 + (n - 1.0) * prob
    return prob, index, int(math.floor(index)), int(math.ceil(index))


def _retain_for(n, index, approx=1e6):
    """lr_retain_links that puts the type-7 index of a block of n long-range pairs at `index` (checked by the caller through _ranks)."""
    return (1.0 - (index - 1.0) / (n - 1.0)) * approx


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
class _Block:
    """One block (1-based inclusive ranges, as mi_all_pairs takes them): its long-range pairs in the reference's row order and their dense
    device MI, computed once and shared by every retain value tried on it."""

    def __init__(self, engine, rng4, POS, g, sr_dist):
        fs, fe, ts, te = rng4
        self.rng4 = rng4
        self.fi, self.ti = np.arange(fs - 1, fe), np.arange(ts - 1, te)
        self.Md = Md = engine.mi_block(self.fi, self.ti)
        rr, cc = orc.block_pair_index(len(self.fi), len(self.ti), fs == ts)
        P = np.asarray(POS, dtype=np.float64)
        lrm = orc.circ_len(P[self.ti][cc], P[self.fi][rr], g) > sr_dist
        self.rr, self.cc = rr[lrm], cc[lrm]
        self.n_sr = int((~lrm).sum())
        self.vals = Md[self.rr, self.cc]
        self.n = len(self.vals)
        self.sorted = np.sort(self.vals)

    def want(self, retain, approx):
        """(a, b, MI, threshold, n_lr) as R/computePairwiseMI.R:352-358 keeps them."""
        if self.n == 0:
            e = np.zeros(0, dtype=np.int64)
            return e, e, np.zeros(0), float("nan"), 0
        thr = orc.quantile7(self.vals, _ranks(self.n, retain, approx)[0])
        keep = self.vals >= thr
        return self.fi[self.rr[keep]], self.ti[self.cc[keep]], self.vals[keep], thr, self.n

    def group(self, a, b):
        """1-based ranks [first, last] of the tie group of the pair of SNPs (a, b) (0-based) among the block's long-range pairs, and its MI."""
        value = self.Md[a - self.fi[0], b - self.ti[0]]
        return int(np.searchsorted(self.sorted, value, "left")) + 1, int(np.searchsorted(self.sorted, value, "right")), value


def _check(got, want, tag):
    (la, lb, lmi), st = got
    off = 0
    for bi, (wa, wb, wmi, thr, n_lr) in enumerate(want):
        n = int(st["n_lr_kept"][bi])
        assert int(st["n_lr_total"][bi]) == n_lr, (tag, bi, int(st["n_lr_total"][bi]), n_lr)
        assert n == len(wmi), (tag, bi, n, len(wmi))
        d = float(st["disc_thresh"][bi])
        assert d == thr or (math.isnan(thr) and math.isnan(d)), (tag, bi, d, thr)
        assert np.array_equal(la[off:off + n], wa) and np.array_equal(lb[off:off + n], wb), (tag, bi)
        assert np.array_equal(lmi[off:off + n].view(np.int64), wmi.view(np.int64)), (tag, bi)
        off += n
    assert off == len(lmi), (tag, off, len(lmi))


def _same(x, y, tag):
    for u, v in zip(x[0], y[0]):
        assert np.array_equal(u, v), tag
    for k in ("n_lr_total", "n_lr_kept", "n_sr"):
        assert np.array_equal(x[1][k], y[1][k]), (tag, k)
    assert np.array_equal(x[1]["disc_thresh"].view(np.int64), y[1]["disc_thresh"].view(np.int64)), tag


def _pass(engine, blocks, sr_dist, retain, approx):
    engine.mi_all_pairs(np.asarray(blocks, dtype=np.int32).reshape(-1, 4), sr_dist, retain, approx)
    return engine.links(1), engine.block_stats()


def _counters(engine):
    s, p = engine.span_report(), engine.path_report()
    return dict(spans=s["spans"], blocks=s["blocks"], redone=s["redone"], spec_misses=p["spec_misses"])


def _run(engine, blks, retain, approx, tag, sr_dist=SR, want=None, deltas=None):
    """The pass over `blks` cold and warm, sort-free and sorting: each == the numpy rule, all four == each other.  Returns the four results;
    `deltas` collects {(select mode, cold): what the pass added to the span and miss counters}."""
    want = [b.want(retain, approx) for b in blks] if want is None else want
    rows = [b.rng4 for b in blks]
    out = []
    try:
        for mode in (0, 1):
            engine.set_select(mode)
            for cold in (True, False):
                if cold:
                    engine.reset_speculation()
                c0 = _counters(engine)
                got = _pass(engine, rows, sr_dist, retain, approx)
                c1 = _counters(engine)
                if deltas is not None:
                    deltas[(mode, cold)] = {k: c1[k] - c0[k] for k in c0}
                _check(got, want, (tag, "select", mode, "cold" if cold else "warm"))
                out.append(got)
    finally:
        engine.set_select(0)
    for g in out[1:]:
        _same(out[0], g, tag)
    return out


# ------------------------------------------------------------------------------------------------
# alignments
# ------------------------------------------------------------------------------------------------
def _columns(rs, n, N):
    """n random two-allele SNP rows over N sequences (minor frequency 0.2 .. 0.5), both alleles present."""
    major = rs.integers(0, 4, n)
    minor = (major + rs.integers(1, 4, n)) % 4
    maf = rs.uniform(0.2, 0.5, n)
    st = np.where(rs.random((n, N)) < maf[:, None], minor[:, None], major[:, None]).astype(np.uint8)
    st[:, 0] = major
    st[:, N - 1] = minor
    return st


def _load(engine, al, POS=None):
    """The alignment with distinct random weights (all-distinct MI values wherever the SNP rows differ), optionally other positions."""
    POS = al["POS"] if POS is None else POS
    engine.set_engine(L.ENGINE_MFMA)
    engine.set_alignment(al["states"])
    uqe = (engine.state_counts() > 0).T.astype(np.float64)
    engine.set_weights(al["hdw"])
    g = float(int(POS.max()) + 3 * STEP)
    engine.set_snp_meta(uqe.sum(axis=1), uqe, POS, np.ones(len(POS), dtype=np.int32), g)
    return POS, g


@pytest.fixture(scope="module")
def wide():
    """2051 unrelated SNPs x 64 sequences: the keep-everything blocks around SEL_MAX."""
    rs = np.random.default_rng(20260)
    st = _columns(rs, 2051, 64)
    return dict(states=st, hdw=rs.uniform(0.25, 1.0, 64), POS=(STEP * (1 + np.arange(len(st)))).astype(np.int32))


# layout of the clone alignment, 0-based SNP index: from side F = [a x 97 | c x 90 | 250 unrelated], to side T = [250 unrelated | b x 64 | d x 90];
# b is a with three sequences flipped (a x b: the top of every block that holds it), c and d are unrelated (c x d: mid-distribution).  No clone pair
# lies on a block's local diagonal (a_loc == b_loc is no pair) as long as the to range starts at T0.
A0, NA, C0, NC, F0, NFO = 0, 97, 97, 90, 187, 250
T0, NTO, B0, NB, D0, ND = 437, 250, 687, 64, 751, 90
LC = 841


@pytest.fixture(scope="module")
def clones():
    rs = np.random.default_rng(20261)
    N = 128
    a, c, d = _columns(rs, 3, N)
    b = a.copy()
    for s in (5, 41, 90):     # three sequences take a's other allele
        b[s] = a[0] if a[s] == a[N - 1] else a[N - 1]
    st = np.concatenate([np.tile(a, (NA, 1)), np.tile(c, (NC, 1)), _columns(rs, NFO, N), _columns(rs, NTO, N), np.tile(b, (NB, 1)), np.tile(d, (ND, 1))])
    assert st.shape == (LC, N)
    return dict(states=st, hdw=rs.uniform(0.25, 1.0, N), POS=(STEP * (1 + np.arange(LC))).astype(np.int32))


def _r(lo0, n):
    """0-based start + count -> the 1-based inclusive range of mi_all_pairs."""
    return lo0 + 1, lo0 + n


# ------------------------------------------------------------------------------------------------
# 1, 2: keep everything; the SEL_MAX boundary
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng4,n_lr", [((1, 1000, 1001, 2000), 999_000), ((1, 1400, 1, 1400), 979_300),
                                       ((1, 1024, 1025, 2049), SEL_MAX)])
def test_keep_everything_dense_bitmap(engine, wide, rng4, n_lr):
    """prob = 0 (lr_links_approx == lr_retain_links): every long-range pair is a candidate and is kept, so every 1024-bit chunk and 65536-bit
    super-chunk of k_sel_scatter's bitmap inside the pair range is full and the rows must come out in exact reference order: an off-diagonal
    block (upper then lower segment, key space 2 nf nt), a diagonal one (lower segment only, keys behind nf nt), and a block of exactly
    SEL_MAX = 2^20 long-range pairs (1024 x 1025 less its 1024 local-diagonal cells), the most the sort-free path takes."""
    POS, g = _load(engine, wide)
    blk = _Block(engine, rng4, POS, g, SR)
    assert blk.n == n_lr <= SEL_MAX and blk.n_sr == 0
    for (_, st) in _run(engine, [blk], 1e6, 1e6, rng4):
        assert int(st["n_lr_total"][0]) == int(st["n_lr_kept"][0]) == n_lr       # candidates == kept == every pair: the bitmap is dense


def test_one_pair_above_sel_max_takes_the_sort_path(engine, wide):
    """2^20 + 1 long-range pairs, all kept: one candidate more than SEL_MAX, so select_rows takes the two radix sorts in both modes.  1025 x 1025
    less the 1025 local-diagonal cells less 1023 short-range pairs (the last from-side SNP sits 1 .. 1023 below the first 1023 to-side ones)."""
    n = len(wide["POS"])
    POS = np.empty(n, dtype=np.int32)
    POS[:1025] = 5000 * (1 + np.arange(1025))
    POS[1025:2048] = POS[1024] + 1 + np.arange(1023)
    POS[2048:] = POS[2047] + 5000 * (1 + np.arange(n - 2048))
    POS, g = _load(engine, wide, POS)
    blk = _Block(engine, (1, 1025, 1026, 2050), POS, g, 1023.5)
    assert blk.n == SEL_MAX + 1 and blk.n_sr == 1023
    for (_, st) in _run(engine, [blk], 1e6, 1e6, "2^20 + 1", sr_dist=1023.5):
        assert int(st["n_lr_kept"][0]) == SEL_MAX + 1 and int(st["n_sr"][0]) == 1023


# ------------------------------------------------------------------------------------------------
# 3: tie groups around SEL_LIST on the threshold
# ------------------------------------------------------------------------------------------------
def _index_at(blk, lo, frac=0.5, approx=1e6):
    """retain with floor(index) == lo and a fractional index (the interpolation runs unless x[hi] == x[lo])."""
    retain = _retain_for(blk.n, lo + frac, approx)
    _, index, lo_, hi_ = _ranks(blk.n, retain, approx)
    assert lo_ == lo and hi_ == lo + 1 and index > lo, (lo, index)
    return retain


def test_tie_group_larger_than_the_lds_list(engine, clones):
    """The whole F x T block: the 90 x 90 copies of (c, d) are 8100 pairs with one MI bit pattern in the middle of the distribution.  Rank lo at the
    group's first element, in its middle, at its last: the bucket of the threshold then holds more than SEL_LIST keys and k_sel_thresh selects
    from the global list.  The group is kept or dropped as one, as the numpy rule says (kept whole at first / middle; at the last element x[hi]
    lies above the group and the interpolated threshold drops it whole)."""
    POS, g = _load(engine, clones)
    blk = _Block(engine, (1, T0, T0 + 1, LC), POS, g, SR)
    first, last, v = blk.group(C0, D0)
    assert last - first + 1 == NC * ND == 8100 > SEL_LIST
    in_group = blk.vals == v
    for where, lo in (("first", first), ("middle", (first + last) // 2), ("last", last)):
        retain = _index_at(blk, lo)
        assert int((_bucket(blk.sorted) == _bucket(blk.sorted[lo - 1])).sum()) > SEL_LIST      # what k_sel_thresh counts: the whole bucket of x[lo]
        wa, wb, wmi, thr, _ = blk.want(retain, 1e6)
        n_in = int((in_group & (blk.vals >= thr)).sum())
        assert n_in == (8100 if where != "last" else 0), (where, n_in)
        _run(engine, [blk], retain, 1e6, ("8100", where))


@pytest.mark.parametrize("n_a", [96, 97])
def test_bucket_population_on_both_sides_of_sel_list(engine, clones, n_a):
    """The copies of (a, b) are the block's largest MI and alone in their bucket: 96 x 64 = 6144 = SEL_LIST keys still fit the LDS list, 97 x 64 =
    6208 do not.  Rank lo inside the group, at its first element, in its middle and at its last but one (hi is then the last rank of the block)."""
    POS, g = _load(engine, clones)
    blk = _Block(engine, (A0 + 1 + (NA - n_a), T0, T0 + 1, LC), POS, g, SR)
    first, last, v = blk.group(A0 + NA - 1, B0)
    size = n_a * NB
    assert last - first + 1 == size and last == blk.n and (size == SEL_LIST if n_a == 96 else size > SEL_LIST)
    assert int((_bucket(blk.sorted) == _bucket(v)).sum()) == size        # nothing else in the bucket: its population is the group
    for lo in (first, (first + last) // 2, last - 1):
        retain = _index_at(blk, lo)
        for (_, st) in _run(engine, [blk], retain, 1e6, (n_a, lo)):
            assert int(st["n_lr_kept"][0]) == size and float(st["disc_thresh"][0]) == v


# ------------------------------------------------------------------------------------------------
# 4: rank hi leaves the bucket of rank lo
# ------------------------------------------------------------------------------------------------
def test_rank_hi_leaves_the_bucket(engine, clones):
    """sel_thresh_body's s_above branch: x[lo] is the largest key of its NBINS bucket and x[hi] the smallest key of any bucket above.  The rank is
    searched on the dense device MI with the restated bucket function; then a variant whose x[hi] equals x[lo] bitwise under a fractional
    index (interpolation skipped), and one whose index is integral (lo == hi)."""
    POS, g = _load(engine, clones)
    blk = _Block(engine, _r(F0, NFO) + _r(T0, NTO), POS, g, SR)          # unrelated x unrelated: every value distinct
    assert len(np.unique(blk.sorted)) == blk.n == NFO * NTO - NFO
    bk = _bucket(blk.sorted)
    edges = np.nonzero(bk[1:] > bk[:-1])[0] + 1          # 1-based rank lo whose successor lies in a higher bucket
    assert len(edges) >= 8, len(edges)
    for lo in (int(edges[len(edges) // 4]), int(edges[len(edges) // 2]), int(edges[-1])):
        assert bk[lo - 1] < bk[lo] and blk.sorted[lo - 1] < blk.sorted[lo]
        assert lo == int((bk <= bk[lo - 1]).sum())                         # the last key of its bucket
        retain = _index_at(blk, lo)
        thr = blk.want(retain, 1e6)[3]
        assert blk.sorted[lo - 1] < thr < blk.sorted[lo]                   # interpolated between the two buckets
        _run(engine, [blk], retain, 1e6, ("edge", lo))
    # x[hi] == x[lo] bitwise, fractional index: inside the group of one unrelated to-side SNP with the 97 copies of a (96 pairs: the copy on the
    # block's local diagonal is no pair)
    big = _Block(engine, (1, T0, T0 + 1, LC), POS, g, SR)
    first, last, v = big.group(A0, T0 + 7)
    assert last - first + 1 >= NA - 1
    retain = _index_at(big, first + 3)
    assert big.sorted[first + 2] == big.sorted[first + 3] and big.want(retain, 1e6)[3] == v
    _run(engine, [big], retain, 1e6, "tie under a fractional index")
    # integral index: prob = 0.5 exactly and n odd
    odd = _Block(engine, _r(F0 + 1, NFO - 1) + _r(T0, NTO), POS, g, SR)
    assert odd.n % 2 == 1
    prob, index, lo, hi = _ranks(odd.n, odd.n / 2, float(odd.n))
    assert prob == 0.5 and lo == hi == (odd.n + 1) // 2 and index == lo
    _run(engine, [odd], odd.n / 2, float(odd.n), "integral index")


# ------------------------------------------------------------------------------------------------
# 5: radix digits
# ------------------------------------------------------------------------------------------------
def _spread(n):
    """type-7 indices from "keep one row" to "keep all but one" (on all-distinct values)."""
    return [n - 0.5, n - 10.5, 0.9 * n + 0.25, 0.5 * n + 0.5, 0.25 * n + 0.75, 0.1 * n + 0.5, 10.5, 1.5]


def test_radix_select_on_few_and_on_all_distinct_values(engine, clones):
    """The six-pass 11-bit radix select: a block of four distinct MI values (copies only: all digits shared inside a group) and a block of all-distinct
    values, eight retain values each from "keep one row" to "keep all but one"; the threshold must be numpy's order statistic (part of every
    _run).  Then a block with exactly one long-range pair."""
    POS, g = _load(engine, clones)
    few = _Block(engine, _r(A0, NA + NC) + _r(B0, NB + ND), POS, g, SR)
    assert len(np.unique(few.sorted)) == 4
    dist = _Block(engine, _r(F0, NFO) + _r(T0, NTO), POS, g, SR)
    assert len(np.unique(dist.sorted)) == dist.n
    for blk, tag in ((few, "few"), (dist, "distinct")):
        kept = []
        for index in _spread(blk.n):
            retain = _retain_for(blk.n, index)
            _, _, lo, hi = _ranks(blk.n, retain, 1e6)
            assert 1 <= lo <= hi <= blk.n and hi == lo + 1
            kept.append(int(_run(engine, [blk], retain, 1e6, (tag, index))[0][1]["n_lr_kept"][0]))
        assert kept == sorted(kept) and kept[0] < kept[-1]
        if tag == "distinct":
            assert kept[0] == 1 and kept[-1] == blk.n - 1
    one = _Block(engine, _r(F0, 1) + _r(T0, 2), POS, g, SR)
    assert one.n == 1
    for retain in (1e6, 3000.0, 0.0):
        for (_, st) in _run(engine, [one], retain, 1e6, ("one pair", retain)):
            assert int(st["n_lr_total"][0]) == int(st["n_lr_kept"][0]) == 1


# ------------------------------------------------------------------------------------------------
# 6: degenerate blocks
# ------------------------------------------------------------------------------------------------
def test_degenerate_blocks(engine, clones):
    """A block without one long-range pair between two ordinary ones (zero rows, NaN threshold, the next block's rows at the right offset); a block
    whose MI is one value; retain = 0 (prob = 1: lo == hi == n, the maximum alone is kept, or its whole tie group)."""
    POS2 = clones["POS"].copy()
    k0 = F0 + NFO - 30                                   # the last 30 unrelated from-side SNPs 1 apart: all within sr_dist of each other
    POS2[k0:F0 + NFO] = POS2[k0] + np.arange(30)
    POS, g = _load(engine, clones, POS2)
    rows = [_r(F0, 60) + _r(T0, 70), _r(k0, 30) + _r(k0, 30), _r(F0 + 60, 50) + _r(T0 + 70, 45)]
    blks = [_Block(engine, r4, POS, g, SR) for r4 in rows]
    assert blks[1].n == 0 and blks[1].n_sr == 30 * 29 // 2 and blks[0].n > 0 and blks[2].n > 0
    retain = _retain_for(blks[0].n, 0.75 * blks[0].n)
    for (_, st) in _run(engine, blks, retain, 1e6, "empty block"):
        assert st["n_lr_total"].tolist() == [blks[0].n, 0, blks[2].n] and int(st["n_lr_kept"][1]) == 0 and int(st["n_sr"][1]) == 435
        assert math.isnan(st["disc_thresh"][1]) and int(st["n_lr_kept"][2]) > 0
    POS, g = _load(engine, clones)
    flat = _Block(engine, _r(A0, NA) + _r(B0, NB), POS, g, SR)
    assert flat.n == NA * NB - NB and flat.sorted[0] == flat.sorted[-1]      # (less the 64 cells of the local diagonal)
    for retain in (_retain_for(flat.n, 0.5 * flat.n + 0.5), 1e6, 0.0):
        for (_, st) in _run(engine, [flat], retain, 1e6, ("one value", retain)):
            assert int(st["n_lr_kept"][0]) == flat.n
    dist = _Block(engine, _r(F0, NFO) + _r(T0, NTO), POS, g, SR)
    assert _ranks(dist.n, 0.0, 1e6)[2:] == (dist.n, dist.n)
    for (_, st) in _run(engine, [dist], 0.0, 1e6, "retain 0"):
        assert int(st["n_lr_kept"][0]) == 1 and float(st["disc_thresh"][0]) == dist.sorted[-1]


# ------------------------------------------------------------------------------------------------
# 7: speculation
# ------------------------------------------------------------------------------------------------
def _sequence(engine, steps, approx=1e6):
    """Passes of one block each on one context WITHOUT reset_speculation in between (one reset in front): each == the numpy rule.  Returns the
    spec_misses every pass added."""
    engine.reset_speculation()
    missed = []
    for blk, retain in steps:
        m0 = engine.path_report()["spec_misses"]
        _check(_pass(engine, [blk.rng4], SR, retain, approx), [blk.want(retain, approx)], ("sequence", blk.rng4, retain))
        missed.append(engine.path_report()["spec_misses"] - m0)
    return missed


def test_speculation_guess_too_high_too_low_and_exact(engine, clones):
    """pick_bucket_body in speculative mode, both selection modes.  (i) A block whose threshold is the MI of the (a, b) copies leaves a guess far above
    every bucket of the unrelated block that follows: `lo <= part[0]`, the block is redone (spec_misses) and must still equal the numpy rule;
    then the reverse order (a guess far below the true bucket).  (ii) The guess itself is not reported; it is bracketed: after a cold block with
    true bucket B1 the guess is B1 - 10 (update_guess), so a block whose true bucket is B1 - 10 must not miss and one at B1 - 11 must."""
    POS, g = _load(engine, clones)
    high = _Block(engine, (1, T0, T0 + 1, LC), POS, g, SR)
    low = _Block(engine, _r(F0, NFO) + _r(T0, NTO), POS, g, SR)
    r_hi, r_lo = _retain_for(high.n, high.n - 500.5), _retain_for(low.n, low.n - 200.5)
    assert max(r_hi, r_lo) < 0.007 * 1e6                                       # both speculate (speculation_pays)
    b_hi, b_lo = int(_bucket([high.want(r_hi, 1e6)[3]])[0]), int(_bucket([low.want(r_lo, 1e6)[3]])[0])
    assert b_hi - GUESS_MARGIN > int(_bucket(low.sorted[-1:])[0]) and b_lo > GUESS_MARGIN      # the guess the high block leaves lies above ALL of the low block
    # (ii) ranks of the unrelated block, inside its speculative range, whose buckets are B1 - 10 and B1 - 11
    bk = _bucket(low.sorted)
    top = low.n - int(0.006 * low.n)                       # 1-based ranks above this keep prob above 0.993
    lo1 = next((r for r in range(low.n - 60, top, -1) if {int(bk[r - 1]) - GUESS_MARGIN, int(bk[r - 1]) - GUESS_MARGIN - 1} <= set(bk[top:r].tolist())), None)
    assert lo1 is not None, bk[top:].tolist()
    B1 = int(bk[lo1 - 1])
    lo_exact = top + 1 + int(np.nonzero(bk[top:] == B1 - GUESS_MARGIN)[0][0])
    lo_below = top + 1 + int(np.nonzero(bk[top:] == B1 - GUESS_MARGIN - 1)[0][-1])
    assert bk[lo_exact - 1] == B1 - GUESS_MARGIN and bk[lo_below - 1] == B1 - GUESS_MARGIN - 1
    r_1, r_exact, r_below = _index_at(low, lo1), _index_at(low, lo_exact), _index_at(low, lo_below)
    assert max(r_1, r_exact, r_below) < 0.007 * 1e6
    try:
        for mode in (0, 1):
            engine.set_select(mode)
            m = _sequence(engine, [(high, r_hi), (low, r_lo), (low, r_lo)])
            assert m[0] == 0 and m[1] >= 1, (mode, m)                           # cold: no guess; then the guess was too high
            _sequence(engine, [(low, r_lo), (high, r_hi), (high, r_hi)])        # the guess far too low: many candidates below the true bucket
            m = _sequence(engine, [(low, r_1), (low, r_exact)])
            assert m == [0, 0], (mode, "B_true == guess", m)
            m = _sequence(engine, [(low, r_1), (low, r_below)])
            assert m[0] == 0 and m[1] >= 1, (mode, "B_true == guess - 1", m)
    finally:
        engine.set_select(0)




# ------------------------------------------------------------------------------------------------
# 8: spans
# ------------------------------------------------------------------------------------------------
S = 2048       # ldw_pass_plan.h, span_candidate: the smallest (square) block a span takes


@pytest.fixture(scope="module")
def row():
    """One block row: a from side of 2048 SNPs and, behind it, the to-side blocks T1, T2, Tlow, T3, T4 of 2048 SNPs each and a ragged last one of
    1000.  The from side starts with 90 copies of c; T2 holds 90 copies of a near-copy of c at b_loc 1000 .. 1089 (off the local diagonal): an
    8100-pair tie group on top of that block.  Every SNP of Tlow carries its minor allele in the last sequence alone: the MI of its pairs, and
    so its threshold, lies far below every other block's."""
    rs = np.random.default_rng(20262)
    N = 128
    n = 7 * S + 1000
    st = _columns(rs, n, N)
    c = st[0].copy()
    d = c.copy()
    for s in (9, 60, 101):
        d[s] = c[0] if c[s] == c[N - 1] else c[N - 1]
    st[:90] = c
    st[2 * S + 1000:2 * S + 1090] = d
    low = st[3 * S:4 * S]
    low[:, 1:N - 1] = low[:, :1]
    return dict(states=st, hdw=rs.uniform(0.25, 1.0, N), POS=(STEP * (1 + np.arange(n))).astype(np.int32), n=n)


def _to(k, row):
    """to-side block k of the row (0 .. 4: T1, T2, Tlow, T3, T4; 5: the ragged one) against the from side."""
    return (1, S, S * (k + 1) + 1, S * (k + 2) if k < 5 else row["n"])


def _span_case(engine, row, ks):
    POS, g = _load(engine, row)
    blks = [_Block(engine, _to(k, row), POS, g, SR) for k in ks]
    tie = blks[ks.index(1)]
    retain = _retain_for(tie.n, tie.n - 4000.5)
    assert retain < 0.007 * 1e6                                               # every block speculates
    first, last, v = tie.group(0, 2 * S + 1000)
    lo = _ranks(tie.n, retain, 1e6)[2]
    assert last - first + 1 == 8100 > SEL_LIST and first <= lo <= last == tie.n
    assert int((_bucket(tie.sorted) == _bucket(tie.sorted[lo - 1:lo])[0]).sum()) > SEL_LIST       # the bucket k_sel_thresh(_span) lists
    return blks, retain, tie


def test_span_segments_against_the_per_block_rule(engine, row):
    """Four square long-range-only blocks of 2048 SNPs (T1, T2, T3, T4) and the ragged last block, which runs as an item of its own behind the
    span.  T2 holds the 8100-pair tie group on its threshold: k_sel_thresh_span selects from the global list there.  Spans on and off: equal to
    each other and to the per-block numpy rule, block_stats included.  The warm sort-free pass alone must have formed one span of four
    segments with no segment redone and no miss — the batched kernels of finish_span ran (a cold pass of blocks this small has no guess to
    plan spans on; with set_select(1) a span goes segment by segment through select_rows)."""
    blks, retain, tie = _span_case(engine, row, [0, 1, 3, 4, 5])
    try:
        engine.set_span(False)
        d_off = {}
        off = _run(engine, blks, retain, 1e6, "spans off", deltas=d_off)
        assert all(d["spans"] == 0 and d["blocks"] == 0 for d in d_off.values()), d_off
        engine.set_span(True)
        d_on = {}
        on = _run(engine, blks, retain, 1e6, "spans on", deltas=d_on)
        assert d_on[(0, False)] == dict(spans=1, blocks=4, redone=0, spec_misses=0), d_on
        for x, y in zip(off, on):
            _same(x, y, "spans on == off")
        assert int(on[1][1]["n_lr_kept"][1]) == 8100
    finally:
        engine.set_span(True, 8)


def test_span_segment_without_candidates_is_redone_in_place(engine, row):
    """T1, T2, Tlow, T3 and the ragged block: the warm span's one guess (left by the ragged block of the pass before) lies far above every bucket
    of Tlow, whose segment lists no candidate and is redone on its own in the middle of the span (finish_span: run_block_alone after
    queue_lr_count); the rows of T3 behind it must start at the right offset.  span_report's `redone` and spec_misses prove the redo."""
    blks, retain, tie = _span_case(engine, row, [0, 1, 2, 3, 5])
    want = [b.want(retain, 1e6) for b in blks]
    b_true = [int(_bucket([w[3]])[0]) for w in want]
    assert int(_bucket(blks[2].sorted[-1:])[0]) < min(b_true[:2] + b_true[3:]) - GUESS_MARGIN, b_true      # ALL of Tlow lies below any guess the others leave
    try:
        engine.set_span(True)
        d_on = {}
        on = _run(engine, blks, retain, 1e6, "low segment", want=want, deltas=d_on)
        d = d_on[(0, False)]
        assert (d["spans"], d["blocks"], d["redone"]) == (1, 4, 1) and d["spec_misses"] >= 1, d_on      # (blocks submitted on the guess T2 left may miss too)
        assert int(on[1][1]["n_lr_kept"][2]) > 0 and int(on[1][1]["n_lr_kept"][3]) > 0
        engine.set_span(False)
        for x, y in zip(_run(engine, blks, retain, 1e6, "low segment, spans off", want=want), on):
            _same(x, y, "spans on == off")
    finally:
        engine.set_span(True, 8)


# ------------------------------------------------------------------------------------------------
# 9: the key space of the bitmap at and above SEL_MAX_SUPER super-chunks
# ------------------------------------------------------------------------------------------------
SEL_MAX_SUPER = 8192       # ldw_mi_select.inc: super-chunks a scatter workgroup scans in LDS


def _n_super(nf, nt):
    """select_rows (ldw_mi_items.inc): super-chunks of the bitmap over the 2 nf nt bits of a block's row-order key space."""
    n_chunks = (2 * nf * nt + 1024 - 1) // 1024 + 1
    return (n_chunks + 64 - 1) // 64


def _want_of_top(Md, fi, ti, retain, approx):
    """_Block.want for an off-diagonal block without short-range pairs whose rank lo lies near the top, without a second copy of the block: the
    order statistics from the values above a cut that provably holds them, the rows by one scan in column-major order (upper segment, then
    lower: orc.block_pair_index order).  The local diagonal (no pair) is overwritten in place."""
    nf, nt = Md.shape
    m = min(nf, nt)
    Md[np.arange(m), np.arange(m)] = -np.inf
    n = nf * nt - m
    prob, index, lo, hi = _ranks(n, retain, approx)
    need = n - lo + 1                       # values at or above x[lo]
    cut = float(Md.max())
    while True:
        cut *= 0.5
        top = Md[Md > cut]
        if len(top) > need or cut < 1e-300:
            break
    assert len(top) > need
    top.sort()
    x = lambda k: top[len(top) - 1 - (n - k)]          # 1-based rank k of the n pairs
    qs = x(lo)
    if index > lo and x(hi) != qs:                      # orc.quantile7
        h = index - lo
        qs = (1 - h) * qs + h * x(hi)
    kb, ka = np.nonzero(Md.T >= qs)                     # by to-side SNP, then from-side SNP: column-major
    up = ka < kb
    ka, kb = np.concatenate([ka[up], ka[~up]]), np.concatenate([kb[up], kb[~up]])
    return fi[ka], ti[kb], Md[ka, kb], float(qs), n


@pytest.mark.parametrize("nt,n_super", [(16383, SEL_MAX_SUPER), (16385, SEL_MAX_SUPER + 1)])
def test_key_space_at_and_above_the_scatter_scan(engine, nt, n_super):
    """16384 x 16383: exactly SEL_MAX_SUPER = 8192 super-chunks, the largest key space the sort-free path takes (k_sel_scatter scans all of
    spre[]); 16384 x 16385: 2 nf nt > 2^29 bits, 8193 super-chunks, so the key space ALONE sends a few hundred candidates to the two radix sorts
    (prep_block accepts blocks up to nf nt < 2^31).  20 x 20 copies of one SNP are the 400 largest MI values and the kept rows; checked
    against the numpy rule on the dense device MI (about 2.1 GB: the one case above the shape ceiling of this file)."""
    nf, N = 16384, 64
    assert _n_super(nf, nt) == n_super and (2 * nf * nt > 1 << 29) == (n_super > SEL_MAX_SUPER)
    rs = np.random.default_rng(20263)
    st = _columns(rs, nf + nt, N)
    st[:20] = st[0]
    st[nf + 5000:nf + 5020] = st[0]                       # a_loc 0 .. 19 against b_loc 5000 .. 5019: off the local diagonal
    al = dict(states=st, hdw=rs.uniform(0.25, 1.0, N), POS=(STEP * (1 + np.arange(nf + nt))).astype(np.int32))
    POS, g = _load(engine, al)
    # the frugal reference is the oracle's rule: on a small block it equals _Block.want
    small = _Block(engine, (1, 300, nf + 4901, nf + 5300), POS, g, SR)
    r_small = _retain_for(small.n, small.n - 150.5)
    for w0, w1 in zip(small.want(r_small, 1e6), _want_of_top(small.Md.copy(order="F"), small.fi, small.ti, r_small, 1e6)):
        assert np.array_equal(np.asarray(w0), np.asarray(w1))
    fi, ti = np.arange(nf), np.arange(nf, nf + nt)
    Md = engine.mi_block(fi, ti)
    n = nf * nt - min(nf, nt)
    retain = _retain_for(n, n - 199.5)
    assert retain < 0.007 * 1e6
    want = _want_of_top(Md, fi, ti, retain, 1e6)
    assert len(want[2]) == 400 and want[3] == Md[0, 5000] and set(want[0].tolist()) == set(range(20))
    # candidates: cold every pair from the threshold's bucket up, warm from the guess (10 buckets below) up — far fewer than SEL_MAX either way
    lo_val = np.array([(int(_bucket([want[3]])[0]) - GUESS_MARGIN + ((1023 - 20) << 7)) << 45], dtype=np.int64).view(np.float64)[0]
    n_cand = int(np.count_nonzero(Md >= lo_val))
    assert 400 <= n_cand <= SEL_MAX, n_cand
    del Md
    blk = type("B", (), dict(rng4=(1, nf, nf + 1, nf + nt)))()
    for (_, stt) in _run(engine, [blk], retain, 1e6, ("key space", nt), want=[want]):
        assert int(stt["n_lr_kept"][0]) == 400 and int(stt["n_lr_total"][0]) == n
