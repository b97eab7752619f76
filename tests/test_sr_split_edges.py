"""The short/long-range split at its geometric edges.  Every pair of a block becomes a short-range row or a long-range candidate by ONE rule of
the reference (R/computePairwiseMI.R:330-333): ``len = 0.5 g - |((pos1 - pos2) %% g) - 0.5 g|``, short-range iff ``len <= sr_dist``, rows in the
order of :306-310, and in SR-only mode a site is first dropped by the strict ``< sr_dist`` (:182-183).  The engine states the rule in six places
("The six statements of the short/long-range rule"): A build_cols (host windows), B k_cols_dev .. k_sr_fill_all (device windows, behind
ldw_sr_pairs_fill), C k_gen_count / k_gen_emit_sr (the predicate per pair), D span_candidate and the quick rejects (four end positions),
E sr_pairs_on_circle (table sizing), F mi._near_mask / mi.lr_links_approx / rcompat.circ_len.  This file ties them to the rule.

The reference isolates the split from the MI arithmetic, as test_lr_select_edges.py does: per block the dense DEVICE MI (``engine.mi_block``) goes
through ``orc.block_pair_index`` / ``orc.circ_len`` / ``orc.block_links`` in numpy, and the pass must reproduce n_sr, n_lr_total, the short-range rows as
a sequence with their MI bits and the long-range rows.  No tolerance anywhere: every comparison is ``==`` / ``np.array_equal``, MI as bits.  g and
sr_dist are integers or multiples of 1/2 and the positions are integers, so every operation of the rule is exact in fp64 in every spelling.  A
non-dyadic g is OUT OF SCOPE: R's ``%%`` on doubles goes through long double, which the oracle does not restate.

Every case asserts on the reference, before it touches the device, that its construction has the property it was built for (pairs at exactly
len == sr_dist directly and across the origin, columns whose partners form two index runs, blocks with no / some / only short-range pairs); a
construction that lacks its property FAILS, it never skips.

Paths seen on the device (path_report, printed by the test): blocks of at most 600 SNPs x 128 sequences at lr_retain_links = 0.004 lr_links_approx
take the approximate path wherever they hold a long-range pair, and the plain path where 2 sr_dist >= g (``test_default_paths_equal_the_rule``
asserts both); spans on the approximate path are reached in the span case.

With the one-turn condition (within_one_turn, ldw_pass_plan.h) taken out of build_cols and ldw_sr_pairs_fill, the four cases of
``test_positions_beyond_one_turn_of_the_circle`` fail and nothing else does: the three with rows on _check's "short-range rows" assertion for
mi_all_pairs (the first call), the fourth because no LDW_ERR_ARG is raised."""
import math
import os

import numpy as np
import pytest

import ldw_oracle as orc
from ldweaver_amd import _lib as L
from ldweaver_amd import mi as MIH
from ldweaver_amd.synth import synth_alignment

gpu = pytest.mark.gpu

LS, NSEQ = 600, 128
CASES = [(60000.0, 2000.0), (60001.0, 2001.0), (60000.5, 2000.5), (60000.0, 0.0), (60000.0, 99.0), (60000.0, 29999.5), (60000.0, 30000.0),
         (60000.0, 45000.0)]
BL128 = [tuple(b) for b in orc.make_blocks(LS, 128)]        # 15 blocks, the last block column ragged (88 SNPs)
BL256 = [tuple(b) for b in orc.make_blocks(LS, 256)]        # POS[255] == POS[256] on both sides of a block boundary
SINGLE = (1, LS, 1, LS)
TO_FIRST = (300, 427, 1, 128)                               # the to side BEFORE the from side
WIDE_A, WIDE_B = (1, LS, 1, 100), (1, LS, 250, 349)         # sides that overlap without being equal; WIDE_B holds 100 pairs of a SNP with itself
EXTRA = [SINGLE, TO_FIRST, WIDE_A, WIDE_B]
# the passes of a case: (blocks, quirk modes).  Both quirk modes where every block is square, the intended mode elsewhere (as the parity tests do)
LISTS = [(BL128, (L.QUIRK_INTENDED,)), (BL256, (L.QUIRK_INTENDED,)), ([SINGLE], (L.QUIRK_INTENDED, L.QUIRK_REFERENCE)), ([TO_FIRST], (L.QUIRK_INTENDED,)),
         ([WIDE_A], (L.QUIRK_INTENDED,))]


def _positions(n, g, step=100):
    """1 + step k, three SNPs at one position inside a block, one position on both sides of the 256-boundary, and the last SNP at floor(g): len 1 to
    the first one across the origin."""
    POS = (1 + step * np.arange(n)).astype(np.int32)
    POS[11] = POS[12] = POS[10]
    POS[256] = POS[255]
    POS[n - 1] = int(math.floor(g))
    assert np.all(np.diff(POS) >= 0) and POS[0] >= 0 and POS[-1] <= g
    return POS


class _Env:
    """An environment switch the library reads per call."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k in self.kw:
            assert k not in os.environ, k
        os.environ.update(self.kw)

    def __exit__(self, *exc):
        for k in self.kw:
            os.environ.pop(k)


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
def _lists(rng4):
    fs, fe, ts, te = rng4
    return np.arange(fs - 1, fe), np.arange(ts - 1, te)


def _split(fi, ti, POS, g, sr_dist):
    """(rr, cc, len, sr) of the block's pairs in the reference's row order."""
    rr, cc = orc.block_pair_index(len(fi), len(ti), len(fi) == len(ti) and bool(np.all(fi == ti)))
    P = np.asarray(POS, dtype=np.float64)
    ln = orc.circ_len(P[ti][cc], P[fi][rr], g)
    return rr, cc, ln, ln <= sr_dist


def _runs(fi, ti, POS, g, sr_dist):
    """Per to-side SNP the number of index runs its partners form on the from side (the predicate over ALL from-side SNPs: what ColInfo holds)."""
    P = np.asarray(POS, dtype=np.float64)
    M = orc.circ_len(P[ti][None, :], P[fi][:, None], g) <= sr_dist
    return (M[0].astype(np.int64) + (M[1:] & ~M[:-1]).sum(axis=0)) if len(fi) else np.zeros(len(ti), dtype=np.int64)


class _Ref:
    """One block: the rule on the dense device MI."""

    def __init__(self, fi, ti, dense, POS, paint, g, sr_dist, retain, approx):
        self.fi, self.ti = fi, ti
        rr, cc, ln, sr = _split(fi, ti, POS, g, sr_dist)
        self.sa, self.sb, self.smi = fi[rr[sr]], ti[cc[sr]], dense[rr[sr], cc[sr]]
        self.slen = ln[sr]
        self.n_pairs, self.n_sr, self.n_lr_total = len(rr), int(sr.sum()), int((~sr).sum())
        bl = orc.block_links(dense, fi, ti, POS, paint, g, sr_dist, retain, approx)
        assert bl.n_lr_total == self.n_lr_total and np.array_equal(bl.sr["a"], self.sa) and np.array_equal(bl.sr["b"], self.sb)
        self.la, self.lb, self.lmi, self.thr = bl.lr["a"], bl.lr["b"], bl.lr["MI"], bl.disc_thresh


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _tables(engine):
    return engine.links(0), engine.links(1), engine.block_stats()


def _check(got, refs, tag, keep_sr=True, sr_only=False):
    (sa, sb, smi), (la, lb, lmi), st = got
    so = lo = 0
    for bi, R in enumerate(refs):
        if keep_sr:     # (the rows first: a misplaced row is then named by the message, before the counts that follow from it)
            n = R.n_sr
            assert np.array_equal(sa[so:so + n], R.sa) and np.array_equal(sb[so:so + n], R.sb), (tag, bi, "short-range rows", _first_diff(sa[so:so + n], sb[so:so + n], R.sa, R.sb))
            assert int(st["n_sr"][bi]) == R.n_sr, (tag, bi, "n_sr", int(st["n_sr"][bi]), R.n_sr)
            assert np.array_equal(_bits(smi[so:so + n]), _bits(R.smi)), (tag, bi, "short-range MI bits")
            so += n
        if not sr_only:
            assert int(st["n_lr_total"][bi]) == R.n_lr_total, (tag, bi, "n_lr_total", int(st["n_lr_total"][bi]), R.n_lr_total)
            n = int(st["n_lr_kept"][bi])
            assert n == len(R.lmi), (tag, bi, "n_lr_kept", n, len(R.lmi))
            d = float(st["disc_thresh"][bi])
            assert d == R.thr or (math.isnan(d) and math.isnan(R.thr)), (tag, bi, d, R.thr)
            assert np.array_equal(la[lo:lo + n], R.la) and np.array_equal(lb[lo:lo + n], R.lb), (tag, bi, "long-range rows", _first_diff(la[lo:lo + n], lb[lo:lo + n], R.la, R.lb))
            assert np.array_equal(_bits(lmi[lo:lo + n]), _bits(R.lmi)), (tag, bi, "long-range MI bits")
            lo += n
    assert so == len(smi) and lo == len(lmi), (tag, "rows behind the last block", so, len(smi), lo, len(lmi))


def _first_diff(a, b, wa, wb):
    """The first row that differs, for the assertion's message: (row, got (a, b), want (a, b))."""
    n = min(len(a), len(wa))
    bad = np.nonzero((np.asarray(a[:n]) != wa[:n]) | (np.asarray(b[:n]) != wb[:n]))[0]
    k = int(bad[0]) if len(bad) else n
    pick = lambda x, y: (int(x[k]), int(y[k])) if k < len(x) else None
    return k, pick(a, b), pick(wa, wb)


def _same(x, y, tag):
    for w in (0, 1):
        for u, v in zip(x[w][:2], y[w][:2]):
            assert np.array_equal(u, v), (tag, w)
        assert np.array_equal(_bits(x[w][2]), _bits(y[w][2])), (tag, w, "MI bits")
    for k in ("n_lr_total", "n_lr_kept", "n_sr"):
        assert np.array_equal(x[2][k], y[2][k]), (tag, k)
    assert np.array_equal(_bits(x[2]["disc_thresh"]), _bits(y[2]["disc_thresh"])), (tag, "disc_thresh")


# ------------------------------------------------------------------------------------------------
# the alignment
# ------------------------------------------------------------------------------------------------
class _Layout:
    """600 SNPs x 128 sequences on the engine, optionally with its SNPs permuted; the dense device MI of a block is computed once per (block, quirk
    mode) — it depends neither on the positions nor on g."""

    def __init__(self, seed, perm=None):
        syn = synth_alignment(LS, NSEQ, seed=seed)
        self.perm = np.arange(LS) if perm is None else perm
        self.states = np.ascontiguousarray(np.asarray(syn["states"])[self.perm])
        self.paint = np.asarray(syn["paint"], dtype=np.int32)[self.perm]
        self.hdw = None
        self.dense = {}

    def load(self, engine, g):
        """The alignment, the engine's Hamming weights and the positions of `g` (permuted with the SNPs).  Returns POS as the engine holds it."""
        engine.set_engine(L.ENGINE_MFMA)
        engine.set_alignment(self.states)
        if self.hdw is None:
            self.hdw = engine.hamming_weights(int(LS * 0.1))
        engine.set_weights(self.hdw)
        uqe = (engine.state_counts() > 0).T.astype(np.float64)
        POS = _positions(LS, g)[self.perm]
        engine.set_snp_meta(uqe.sum(axis=1), uqe, POS, self.paint, g)
        return POS

    def mi(self, engine, fi, ti, quirk):
        key = (fi.tobytes(), ti.tobytes(), quirk)
        if key not in self.dense:
            self.dense[key] = engine.mi_block(fi, ti, quirk)
        return self.dense[key]

    def refs(self, engine, blocks, quirk, POS, g, sr_dist, retain, approx):
        return [_Ref(*_lists(b), self.mi(engine, *_lists(b), quirk), POS, self.paint, g, sr_dist, retain, approx) for b in blocks]


@pytest.fixture(scope="module")
def lay():
    return _Layout(seed=20270)


def _approx(POS, g, sr_dist):
    """lr_links_approx as the driver computes it; 1 where no pair of the alignment is long-range (2 sr_dist >= g: the library refuses 0, and no block
    has a long-range pair to filter)."""
    v = MIH.lr_links_approx(POS, g, sr_dist)
    assert v > 0 or 2 * sr_dist >= g
    return v if v > 0 else 1.0


# ------------------------------------------------------------------------------------------------
# the construction has what each case is there for (the oracle alone)
# ------------------------------------------------------------------------------------------------
def _properties(POS, g, sr_dist, blocks):
    P = np.asarray(POS, dtype=np.float64)
    out = dict(boundary_direct=0, boundary_wrap=0, sr_wrap=0, two_runs=0, max_runs=0, kinds=set())
    for b in blocks:
        fi, ti = _lists(b)
        rr, cc, ln, sr = _split(fi, ti, POS, g, sr_dist)
        direct = np.abs(P[ti][cc] - P[fi][rr])
        at = ln == sr_dist
        out["boundary_direct"] += int((at & (direct == ln)).sum())
        out["boundary_wrap"] += int((at & (direct != ln)).sum())
        out["sr_wrap"] += int((sr & (direct > sr_dist)).sum())        # short-range only because the genome is a circle
        runs = _runs(fi, ti, POS, g, sr_dist)
        out["two_runs"] += int((runs >= 2).sum())
        out["max_runs"] = max(out["max_runs"], int(runs.max()))
        out["kinds"].add("none" if not sr.any() else ("all" if sr.all() else "mixed"))
    return out


# what each (g, sr_dist) is there for: counts that must be >= 1, and the block kinds that must occur (== for the last two: EVERY block all short-range)
WANT = {
    (60000.0, 2000.0): (("boundary_direct", "boundary_wrap", "sr_wrap", "two_runs"), {"mixed", "none"}),
    (60001.0, 2001.0): (("boundary_wrap", "sr_wrap", "two_runs"), {"mixed", "none"}),                # odd g
    (60000.5, 2000.5): (("boundary_wrap", "sr_wrap", "two_runs"), {"mixed", "none"}),                # non-integral g: A instead of B
    (60000.0, 0.0): (("boundary_direct",), {"mixed", "none"}),                                       # only repeated positions are short-range
    (60000.0, 99.0): (("sr_wrap", "two_runs"), {"mixed", "none"}),                                   # below the grid step: the repeats and the SNP at floor(g)
    (60000.0, 29999.5): (("sr_wrap", "two_runs"), {"all", "mixed"}),                                 # just below g / 2
    (60000.0, 30000.0): (("boundary_direct",), {"all"}),                                             # == g / 2: `2 sr_dist < g` is false
    (60000.0, 45000.0): ((), {"all"}),                                                               # above g / 2
}


def _case(g, sr_dist):
    POS = _positions(LS, g)
    pr = _properties(POS, g, sr_dist, BL128 + EXTRA)
    print(f"g {g} sr_dist {sr_dist}: {pr}")
    counts, kinds = WANT[(g, sr_dist)]
    for k in counts:
        assert pr[k] >= 1, (g, sr_dist, k, pr)
    assert pr["kinds"] >= kinds and (kinds != {"all"} or pr["kinds"] == kinds), (g, sr_dist, pr)
    assert pr["max_runs"] <= 3, pr
    if sr_dist == 0.0:
        assert pr["boundary_wrap"] == 0 and pr["sr_wrap"] == 0 and pr["two_runs"] == 0, pr
    return pr


@pytest.mark.parametrize("g,sr_dist", CASES)
def test_the_construction_has_its_properties(g, sr_dist):
    """No device: the properties on the oracle alone, so that a CPU-only run sees a broken construction too."""
    _case(g, sr_dist)


# ------------------------------------------------------------------------------------------------
# 1, 6: the pass against the reference, every long-range pair kept; keep_sr = False
# ------------------------------------------------------------------------------------------------
def _pass(engine, blocks, sr_dist, retain, approx, quirk, **kw):
    engine.mi_all_pairs(np.asarray(blocks, dtype=np.int32).reshape(-1, 4), sr_dist, retain, approx, quirk=quirk, **kw)
    return _tables(engine)


def _each_pair_once(got, refs, tag):
    """Over a pass whose blocks hold every unordered pair of the alignment at most once (make_blocks, the single block) and that keeps every
    long-range pair: every pair of every block lies in exactly one of the two tables, exactly once.  (The pairs of a block are the reference's:
    an off-diagonal block has no pair on its LOCAL diagonal, :309, so the pass holds L (L - 1) / 2 less min(nf, nt) per off-diagonal block.)"""
    (sa, sb, _), (la, lb, _), _ = got
    a, b = np.concatenate([sa, la]).astype(np.int64), np.concatenate([sb, lb]).astype(np.int64)
    key = np.minimum(a, b) * LS + np.maximum(a, b)
    n_pairs = sum(R.n_pairs for R in refs)
    off_diag = sum(min(len(R.fi), len(R.ti)) for R in refs if not (len(R.fi) == len(R.ti) and np.all(R.fi == R.ti)))
    assert n_pairs == LS * (LS - 1) // 2 - off_diag, (tag, n_pairs, off_diag)
    assert len(key) == n_pairs and len(np.unique(key)) == len(key) and np.all(a != b), (tag, len(key), len(np.unique(key)), n_pairs)


@gpu
@pytest.mark.parametrize("g,sr_dist", CASES)
def test_pass_keeping_every_pair_equals_the_rule(engine, lay, g, sr_dist):
    """lr_retain_links == lr_links_approx: prob = 0 up to the rounding of :348 (1 - ((retain * (n / approx)) / n) is 0 or one ulp of 1, and with the
    latter the type-7 threshold lies a hair above the block's minimum, which is then dropped: whatever orc.block_links says holds).  Per block n_sr,
    n_lr_total, the short-range rows as a sequence with MI bits, the long-range rows as orc.block_links gives them.  Then lr_retain_links = 2
    lr_links_approx, where max(0, .) makes prob 0 exactly: every long-range pair is kept, BOTH tables are the whole split, and over the pass every
    pair lies in exactly one of them once.  Then keep_sr = False: the long-range table and n_lr_total unchanged, the short-range table empty."""
    _case(g, sr_dist)
    POS = lay.load(engine, g)
    approx = _approx(POS, g, sr_dist)
    for blocks, quirks in LISTS:
        for quirk in quirks:
            tag = (g, sr_dist, blocks[0], len(blocks), quirk)
            refs = lay.refs(engine, blocks, quirk, POS, g, sr_dist, approx, approx)
            _check(_pass(engine, blocks, sr_dist, approx, approx, quirk), refs, tag)
            refs = lay.refs(engine, blocks, quirk, POS, g, sr_dist, 2 * approx, approx)
            got = _pass(engine, blocks, sr_dist, 2 * approx, approx, quirk)
            _check(got, refs, tag + ("prob 0",))
            assert all(len(R.lmi) == R.n_lr_total for R in refs), tag                     # (kept everything: the partition below is whole)
            if blocks in (BL128, BL256, [SINGLE]):
                _each_pair_once(got, refs, tag)
            lr_only = _pass(engine, blocks, sr_dist, 2 * approx, approx, quirk, keep_sr=False)
            _check(lr_only, refs, tag + ("keep_sr=False",), keep_sr=False)
            assert len(lr_only[0][2]) == 0, tag
            for w in range(3):
                assert np.array_equal(lr_only[1][w], got[1][w]), tag
            assert np.array_equal(lr_only[2]["n_lr_total"], got[2]["n_lr_total"]), tag


# ------------------------------------------------------------------------------------------------
# 2: the speculative default, verify mode, the plain path and the histogram engine
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("g,sr_dist", CASES)
def test_default_paths_equal_the_rule(engine, lay, g, sr_dist):
    """lr_retain_links = 0.004 lr_links_approx, the speculative default: cold (reset_speculation), warm, verify mode (set_screen(2): no new
    screen_violations), the plain path (set_path(1), set_screen(0), set_mixed(0)) and ENGINE_HIST all equal the reference, and so each other, bit for
    bit.  path_report before and after the cold and the warm pass is printed.  Seen on the MI355X and asserted: blocks this small DO open the
    approximate path wherever a long-range pair exists (apx gate "ok"; of the 30 block runs of the 15-block list 27 to 29 are counted as approximate,
    the rest are blocks without a long-range pair and blocks redone on the plain path after a wrong guess); where 2 sr_dist >= g no block has a
    long-range pair and every block is counted as plain, once per pass."""
    _case(g, sr_dist)
    POS = lay.load(engine, g)
    approx = _approx(POS, g, sr_dist)
    retain = 0.004 * approx
    try:
        for blocks, quirks in LISTS:
            quirk = quirks[0]
            tag = (g, sr_dist, blocks[0], len(blocks))
            refs = lay.refs(engine, blocks, quirk, POS, g, sr_dist, retain, approx)
            p0 = engine.path_report()
            engine.reset_speculation()
            cold = _pass(engine, blocks, sr_dist, retain, approx, quirk)
            _check(cold, refs, tag + ("cold",))
            _check(_pass(engine, blocks, sr_dist, retain, approx, quirk), refs, tag + ("warm",))
            p1 = engine.path_report()
            took = {k: p1[k] - p0[k] for k in ("apx_blocks", "mixed_blocks", "plain_blocks", "probe_blocks", "spec_misses")}
            print(f"g {g} sr_dist {sr_dist} blocks {blocks[0]} x{len(blocks)}: {took} gate {p1['apx_gate']!r}")
            if 2 * sr_dist < g:
                assert took["apx_blocks"] >= 1 and p1["apx_gate"] == "ok", (tag, took, p1["apx_gate"])
            else:
                assert took["apx_blocks"] == 0 and took["plain_blocks"] == 2 * len(blocks), (tag, took)
            engine.set_screen(2)
            v0 = engine.counters()["screen_violations"]
            _check(_pass(engine, blocks, sr_dist, retain, approx, quirk), refs, tag + ("verify",))
            assert engine.counters()["screen_violations"] - v0 == 0, tag
            engine.set_screen(0); engine.set_mixed(False); engine.set_path(1)
            plain = _pass(engine, blocks, sr_dist, retain, approx, quirk)
            _check(plain, refs, tag + ("plain",))
            _same(cold, plain, tag)
            engine.set_mixed(True); engine.set_screen(1); engine.set_path(0)
            engine.set_engine(L.ENGINE_HIST)
            _check(_pass(engine, blocks, sr_dist, retain, approx, quirk), refs, tag + ("ENGINE_HIST",))
            engine.set_engine(L.ENGINE_MFMA)
    finally:
        engine.set_engine(L.ENGINE_MFMA)
        engine.set_mixed(True); engine.set_screen(1); engine.set_path(0)


# ------------------------------------------------------------------------------------------------
# 3: Engine.sr_pairs, on the device and on the host
# ------------------------------------------------------------------------------------------------
def _sr_pairs_equal(engine, blocks, sr_dist, wa, wb, tag):
    """The count-only call (it sizes the outputs inside Engine.sr_pairs) and the filled (a, b), by k_cols_dev .. k_sr_fill_all where g is integral
    and by build_cols / k_sr_fill with LDW_SR_PAIRS_HOST=1 (a non-integral g takes the latter by itself)."""
    bl = np.asarray(blocks, dtype=np.int32).reshape(-1, 4)
    for env in ({}, dict(LDW_SR_PAIRS_HOST="1")):
        with _Env(**env):
            a, b = engine.sr_pairs(bl, sr_dist)
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert len(a) == len(wa), (tag, env, "rows", len(a), len(wa))
        assert np.array_equal(a, wa) and np.array_equal(b, wb), (tag, env, "short-range rows", _first_diff(a, b, wa, wb))


@gpu
@pytest.mark.parametrize("g,sr_dist", CASES)
def test_sr_pairs_equals_the_rule(engine, lay, g, sr_dist):
    _case(g, sr_dist)
    POS = lay.load(engine, g)
    for blocks in (BL128, BL256, [SINGLE], [TO_FIRST, WIDE_A], BL128 + [TO_FIRST]):
        rows = [_split(*_lists(b), POS, g, sr_dist) for b in blocks]
        wa = np.concatenate([_lists(b)[0][rr[sr]] for b, (rr, cc, ln, sr) in zip(blocks, rows)])
        wb = np.concatenate([_lists(b)[1][cc[sr]] for b, (rr, cc, ln, sr) in zip(blocks, rows)])
        _sr_pairs_equal(engine, blocks, sr_dist, wa, wb, (g, sr_dist, blocks[0], len(blocks)))


# ------------------------------------------------------------------------------------------------
# 4: SR-only mode
# ------------------------------------------------------------------------------------------------
def _kp(pos_x, pos_other, g, sr_dist, strict=True):
    """R/computePairwiseMI.R:182-183, literally: sapply(POS_x, function(x) any(abs(0.5 g - abs((POS_other - x) %% g - 0.5 g)) < sr_dist))."""
    keep = np.zeros(len(pos_x), dtype=bool)
    for k, x in enumerate(pos_x):
        v = np.abs(0.5 * g - np.abs(np.mod(pos_other - x, g) - 0.5 * g))
        keep[k] = np.any(v < sr_dist) if strict else np.any(v <= sr_dist)
    return keep


@gpu
@pytest.mark.parametrize("g,sr_dist", [(60000.0, 2000.0), (60001.0, 2001.0), (60000.5, 2000.5), (60000.0, 0.0), (60000.0, 99.0), (60000.0, 30000.0)])
def test_sr_only_drops_sites_by_the_strict_rule(engine, lay, g, sr_dist):
    """SR-only: the sites of a block are first filtered by the STRICT `< sr_dist` (mi._near_mask == the literal restatement), then the block of the
    kept sites is split by `<=`.  A site whose only partners sit at exactly sr_dist is kept by `<=` and dropped by `<`: for (60000, 2000) at least one
    block loses such a site, and its boundary pair, a row of the full pass, is absent here.  sr_dist = 0: every site is dropped, every block skipped,
    both tables empty."""
    _case(g, sr_dist)
    POS = lay.load(engine, g)
    P = POS.astype(np.float64)
    blocks = BL128 + [TO_FIRST, WIDE_A]
    todo, lost = [], []
    for b in blocks:
        fi, ti = _lists(b)
        kf, kt = _kp(P[fi], P[ti], g, sr_dist), _kp(P[ti], P[fi], g, sr_dist)
        nf, nt = MIH._near_mask(P[fi], P[ti], g, sr_dist)
        assert np.array_equal(kf, nf) and np.array_equal(kt, nt), (b, "mi._near_mask")
        gone = fi[_kp(P[fi], P[ti], g, sr_dist, strict=False) & ~kf]
        if kf.any() and kt.any():
            todo.append((fi[kf], ti[kt]))
            lost.append((len(todo) - 1, b, gone))
    if sr_dist == 0.0:
        assert not todo                                          # the strict filter drops every site of every block: as the driver, a pass without one
        engine.links_begin(1)
        engine.links_end()
        assert engine.links_count(0) == 0 and engine.links_count(1) == 0
        return
    assert len(todo) >= 3
    refs = [_Ref(fk, tk, lay.mi(engine, fk, tk, L.QUIRK_INTENDED), POS, lay.paint, g, sr_dist, 1.0, 1.0) for fk, tk in todo]
    engine.links_begin(max(1, len(todo)))
    for fk, tk in todo:
        engine.mi_block_links(fk, tk, sr_dist=sr_dist, sr_only=True, quirk=L.QUIRK_INTENDED)
    engine.links_end()
    got = _tables(engine)
    _check(got, refs, (g, sr_dist, "SR-only"), sr_only=True)
    assert len(got[1][2]) == 0 and engine.links_count(1) == 0     # the long-range table stays empty
    n_lost = sum(len(gone) for _, _, gone in lost)
    print(f"g {g} sr_dist {sr_dist}: {len(todo)} of {len(blocks)} blocks run, {n_lost} from-side sites kept by <= and dropped by <")
    if (g, sr_dist) == (60000.0, 2000.0):
        assert n_lost >= 1
        k, b, gone = next(x for x in lost if len(x[2]))
        fi, ti = _lists(b)
        rr, cc, ln, sr = _split(fi, ti, POS, g, sr_dist)
        s = int(gone[0])
        full = sr & (fi[rr] == s)
        assert full.any() and np.all(ln[full] == sr_dist)          # in the full pass the site has short-range rows, all at the boundary (case 1 checks them)
        assert not np.any(refs[k].sa == s)                        # ... and none here (refs[k] == the device's rows, checked above)


# ------------------------------------------------------------------------------------------------
# 5: positions that do not ascend: the predicate per pair (k_gen_count / k_gen_emit_sr)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lay_perm():
    return _Layout(seed=20270, perm=np.random.default_rng(20271).permutation(LS))


@gpu
@pytest.mark.parametrize("g,sr_dist", [(60000.0, 2000.0), (60001.0, 2001.0)])
def test_permuted_snps_take_the_predicate_itself(engine, lay_perm, g, sr_dist):
    """States, r, uqe, paint and POS permuted together by one fixed permutation: no block's lists ascend, so every block takes the generic path,
    which evaluates the rule per pair on the device.  Keep-everything and the 0.004 default against the reference; sr_pairs refuses (LDW_ERR_STATE)."""
    _case(g, sr_dist)
    POS = lay_perm.load(engine, g)
    assert all(np.any(np.diff(POS[s - 1:e]) < 0) for s, e in {(b[0], b[1]) for b in BL128})
    approx = _approx(POS, g, sr_dist)
    for retain in (approx, 2 * approx, 0.004 * approx):
        refs = lay_perm.refs(engine, BL128, L.QUIRK_INTENDED, POS, g, sr_dist, retain, approx)
        assert sum(R.n_sr for R in refs) > 0 and any(np.any(R.slen == sr_dist) for R in refs)
        engine.reset_speculation()
        got = _pass(engine, BL128, sr_dist, retain, approx, L.QUIRK_INTENDED)
        _check(got, refs, (g, sr_dist, "permuted", retain))
        _check(_pass(engine, BL128, sr_dist, retain, approx, L.QUIRK_INTENDED), refs, (g, sr_dist, "permuted, warm", retain))
        if retain == 2 * approx:     # prob = 0 exactly (test_pass_keeping_every_pair_equals_the_rule)
            assert all(len(R.lmi) == R.n_lr_total for R in refs)
            _each_pair_once(got, refs, (g, sr_dist, "permuted"))
    with pytest.raises(L.LdwError) as e:
        engine.sr_pairs(np.asarray(BL128, dtype=np.int32), sr_dist)
    assert e.value.code == L.LDW_ERR_STATE, e.value


# ------------------------------------------------------------------------------------------------
# blocks whose sides overlap without being equal
# ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("g,sr_dist", [(60000.0, 2000.0), (60000.0, 0.0), (60000.5, 2000.5), (60000.0, 30000.0)])
def test_a_block_that_holds_pairs_of_a_snp_with_itself(engine, lay, g, sr_dist):
    """(1, 600, 250, 349): the to side lies inside the from side, so the block holds 100 pairs of a SNP with itself at len 0 (and both orders of 4950
    pairs).  The reference's else-branch (:309) treats them by local index like any other pair: short-range rows for every sr_dist >= 0."""
    POS = lay.load(engine, g)
    approx = _approx(POS, g, sr_dist)
    fi, ti = _lists(WIDE_B)
    rr, cc, ln, sr = _split(fi, ti, POS, g, sr_dist)
    own = fi[rr] == ti[cc]
    assert int(own.sum()) == 100 and np.all(ln[own] == 0) and np.all(sr[own])
    for retain in (approx, 0.004 * approx):
        refs = lay.refs(engine, [WIDE_B], L.QUIRK_INTENDED, POS, g, sr_dist, retain, approx)
        assert int((refs[0].sa == refs[0].sb).sum()) == 100
        engine.reset_speculation()
        _check(_pass(engine, [WIDE_B], sr_dist, retain, approx, L.QUIRK_INTENDED), refs, (g, sr_dist, "overlap", retain))
        _check(_pass(engine, [WIDE_B], sr_dist, retain, approx, L.QUIRK_INTENDED), refs, (g, sr_dist, "overlap, warm", retain))
    _sr_pairs_equal(engine, [WIDE_B], sr_dist, refs[0].sa, refs[0].sb, (g, sr_dist, "overlap"))


# ------------------------------------------------------------------------------------------------
# positions beyond one turn of the circle
# ------------------------------------------------------------------------------------------------
G_TURN, SR_TURN = 1000.0, 50.0
# (positions, block, (from position, to position) that looks short-range to the position windows and is long-range by the rule)
TURNS = {
    # to position 2500: its wrap-low window [0, ub(1550)) begins on 500 (len 0) and ends on 1480 (len 20) with 900 (len 400) inside
    "wrap-low": ([500, 900, 1480, 1700, 2460, 2500, 2610, 2720, 2830, 2940], (1, 5, 6, 10), (900, 2500)),
    # to position 1500: its wrap-high window [lb(2450), nf) begins on 2460 (len 40) and ends on 4490 (len 10) with 3900 (len 400) inside
    "wrap-high": ([1480, 1500, 2460, 3500, 3900, 4490], (3, 6, 2, 2), (3900, 1500)),
    "wrap-high, diagonal": ([1480, 1500, 2460, 3500, 3900, 4490], (1, 6, 1, 6), (3900, 1500)),
    # to position 3500: partners 500, 1480, 2460, 3490 with 900, 1700, 2700 between them
    "four runs": ([500, 900, 1480, 1700, 2460, 2700, 3490, 3500, 3610, 3720], (1, 7, 8, 10), None),
}


@gpu
@pytest.mark.parametrize("name", list(TURNS))
def test_positions_beyond_one_turn_of_the_circle(engine, name):
    """ldw_set_snp_meta does not bound POS by g and the reference gives any positions a defined answer (%% folds them).  Where the positions of a block
    span two turns or more, a position WINDOW can begin and end on true partners and hold non-partners inside, and the boundary checks of build_cols
    / k_cols_dev pass: such a block must build every column from the predicate (within_one_turn, ldw_pass_plan.h).  As one block of mi_all_pairs,
    through mi_block_links, and through sr_pairs on the device and on the host (g is integral: without the condition k_cols_dev would serve it).
    Which outcome to expect is decided from the run count of the oracle's own matrix: up to three runs per column the reference's rows, more the
    documented LDW_ERR_ARG, after which the engine serves the next call."""
    pos, blk, wrong = TURNS[name]
    POS = np.asarray(pos, dtype=np.int32)
    n = len(POS)
    assert np.all(np.diff(POS) >= 0) and POS.max() - POS.min() >= G_TURN            # ascending (sr_pairs takes it), beyond one turn
    rs = np.random.default_rng(20272)
    major = rs.integers(0, 4, n)
    minor = (major + rs.integers(1, 4, n)) % 4
    st = np.where(rs.random((n, 64)) < 0.4, minor[:, None], major[:, None]).astype(np.uint8)
    st[:, 0], st[:, 63] = major, minor
    engine.set_engine(L.ENGINE_MFMA)
    engine.set_alignment(st)
    engine.set_weights(rs.uniform(0.25, 1.0, 64))
    uqe = (engine.state_counts() > 0).T.astype(np.float64)
    paint = np.ones(n, dtype=np.int32)
    engine.set_snp_meta(uqe.sum(axis=1), uqe, POS, paint, G_TURN)
    fi, ti = _lists(blk)
    runs = _runs(fi, ti, POS, G_TURN, SR_TURN)
    print(f"{name}: index runs per to-side SNP {runs.tolist()}")
    approx = 100.0
    bl = np.asarray([blk], dtype=np.int32)
    if runs.max() > 3:
        assert name == "four runs"
        for call in (lambda: engine.mi_all_pairs(bl, SR_TURN, approx, approx, quirk=L.QUIRK_INTENDED), lambda: engine.sr_pairs(bl, SR_TURN)):
            with pytest.raises(L.LdwError, match="more than three index runs") as e:
                call()
            assert e.value.code == L.LDW_ERR_ARG, e.value
        with _Env(LDW_SR_PAIRS_HOST="1"), pytest.raises(L.LdwError, match="more than three index runs"):
            engine.sr_pairs(bl, SR_TURN)
        # the engine is usable afterwards: a block of the same alignment whose columns have at most three runs
        blk = (1, 6, 8, 10)
        fi, ti = _lists(blk)
        assert _runs(fi, ti, POS, G_TURN, SR_TURN).max() == 3
        bl = np.asarray([blk], dtype=np.int32)
    else:
        assert name != "four runs" and runs.max() >= 2
    ref = _Ref(fi, ti, engine.mi_block(fi, ti, L.QUIRK_INTENDED), POS, paint, G_TURN, SR_TURN, approx, approx)
    assert ref.n_sr >= 2 and ref.n_lr_total >= 1
    if wrong is not None:      # the pair the windows misplace is a long-range row of the reference
        pa, pb = wrong
        assert np.any((POS[ref.la] == pa) & (POS[ref.lb] == pb)) and not np.any((POS[ref.sa] == pa) & (POS[ref.sb] == pb))
    got = _pass(engine, bl, SR_TURN, approx, approx, L.QUIRK_INTENDED)
    _check(got, [ref], (name, "mi_all_pairs"))
    engine.links_begin(1)
    engine.mi_block_links(fi, ti, sr_dist=SR_TURN, lr_retain_links=approx, lr_links_approx=approx, quirk=L.QUIRK_INTENDED)
    engine.links_end()
    _check(_tables(engine), [ref], (name, "mi_block_links"))
    _sr_pairs_equal(engine, bl, SR_TURN, ref.sa, ref.sb, (name, "sr_pairs"))


# ------------------------------------------------------------------------------------------------
# spans at the boundary of span_candidate
# ------------------------------------------------------------------------------------------------
SPAN_L, SPAN_B = 10240, 2048


@pytest.fixture(scope="module")
def span_al(engine):
    syn = synth_alignment(SPAN_L, NSEQ, seed=20273)
    st = np.ascontiguousarray(np.asarray(syn["states"]))
    engine.set_engine(L.ENGINE_MFMA)
    engine.set_alignment(st)
    return dict(states=st, hdw=engine.hamming_weights(int(SPAN_L * 0.1)), paint=np.asarray(syn["paint"], dtype=np.int32),
                POS=(1 + np.arange(SPAN_L)).astype(np.int32))


def _n_sr_of(b, POS, g, sr_dist):
    """Short-range rows of a SQUARE block by the rule, without the pair index arrays."""
    fi, ti = _lists(b)
    P = POS.astype(np.float64)
    M = orc.circ_len(P[ti][None, :], P[fi][:, None], g) <= sr_dist
    return int(np.tril(M, -1).sum()) if b[0] == b[2] else int(M.sum() - np.trace(M))


@gpu
@pytest.mark.parametrize("g,sr_dist", [(12288.0, 2048.0), (12287.0, 2048.0), (12288.0, 2049.0)])
def test_spans_at_the_boundary_of_span_candidate(engine, span_al, g, sr_dist):
    """10240 SNPs one apart in five blocks of 2048.  sr_dist = 2048: the nearest pair of every block (i, i + 2) is 2049 apart, so these blocks hold no
    short-range pair and may join spans.  Block (1, 5) closes the circle at pf_min + g - pt_max = g - 10239: with g = 12288 it holds none either; with g
    = 12287 the pair (SNP 1, SNP 10240) sits at len == sr_dist: exactly one short-range row, the dense block's MI bits, and the block an item of its own.
    sr_dist = 2049 with g = 12288: every block (i, i + 2) (and (1, 5)) holds exactly one boundary row and no span may take it.  The speculative default
    cold and warm (the warm pass has a guess to plan spans on) against the plain path, bit for bit; n_sr per block against the rule."""
    POS = span_al["POS"]
    engine.set_engine(L.ENGINE_MFMA)
    engine.set_alignment(span_al["states"])
    engine.set_weights(span_al["hdw"])
    uqe = (engine.state_counts() > 0).T.astype(np.float64)
    engine.set_snp_meta(uqe.sum(axis=1), uqe, POS, span_al["paint"], g)
    blocks = [tuple(b) for b in orc.make_blocks(SPAN_L, SPAN_B)]
    assert len(blocks) == 15 and blocks[4] == (1, SPAN_B, 4 * SPAN_B + 1, SPAN_L)
    want_sr = [_n_sr_of(b, POS, g, sr_dist) for b in blocks]
    apart2 = [k for k, b in enumerate(blocks) if b[2] - b[0] == 2 * SPAN_B]
    assert len(apart2) == 3
    edge = 1 if sr_dist == 2049.0 else 0
    assert [want_sr[k] for k in apart2] == [edge] * 3 and want_sr[4] == (1 if (g, sr_dist) != (12288.0, 2048.0) else 0), want_sr
    approx = MIH.lr_links_approx(POS, g, sr_dist)
    retain = 0.004 * approx
    try:
        engine.set_screen(0); engine.set_mixed(False); engine.set_path(1)
        plain = _pass(engine, blocks, sr_dist, retain, approx, L.QUIRK_REFERENCE)
        engine.set_mixed(True); engine.set_screen(1); engine.set_path(0)
        assert plain[2]["n_sr"].tolist() == want_sr, (plain[2]["n_sr"].tolist(), want_sr)
        s0, p0 = engine.span_report(), engine.path_report()
        engine.reset_speculation()
        cold = _pass(engine, blocks, sr_dist, retain, approx, L.QUIRK_REFERENCE)
        warm = _pass(engine, blocks, sr_dist, retain, approx, L.QUIRK_REFERENCE)
        s1, p1 = engine.span_report(), engine.path_report()
    finally:
        engine.set_mixed(True); engine.set_screen(1); engine.set_path(0)
    print(f"g {g} sr_dist {sr_dist}: spans {s1['spans'] - s0['spans']} of {s1['blocks'] - s0['blocks']} blocks, apx blocks {p1['apx_blocks'] - p0['apx_blocks']}, n_sr {want_sr}")
    _same(plain, cold, (g, sr_dist, "cold"))
    _same(plain, warm, (g, sr_dist, "warm"))
    assert p1["apx_blocks"] > p0["apx_blocks"], p1["apx_gate"]
    d_spans, d_blocks = s1["spans"] - s0["spans"], s1["blocks"] - s0["blocks"]
    if sr_dist == 2048.0:
        # per pass that plans spans: (1,3) (1,4) [(1,5) only where it holds no short-range row] and (2,4) (2,5); the warm pass does, the cold one may
        per = 5 if g == 12288.0 else 4
        assert (d_spans, d_blocks) in ((2, per), (4, 2 * per)), (s0, s1)
    else:
        assert (d_spans, d_blocks) == (0, 0), (s0, s1)              # the candidates left, (1,4) and (2,5), have no candidate beside them
    # the one row across the origin
    sa, sb, smi = warm[0]
    at = np.nonzero((sa == 0) & (sb == SPAN_L - 1))[0]
    if want_sr[4] == 1:
        fi, ti = _lists(blocks[4])
        dense = engine.mi_block(fi, ti)
        assert len(at) == 1 and _bits(smi[at])[0] == _bits(dense[0, SPAN_B - 1:SPAN_B])[0]
        assert int(at[0]) == sum(want_sr[:4])                         # the only row of block 4, at its place in the table
    else:
        assert len(at) == 0


# ------------------------------------------------------------------------------------------------
# the Python mirror (no GPU; the built library for r_sample only)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [240000.0, 240001.0])
def test_lr_links_approx_fast_and_slow_path_against_the_oracle(g):
    """mi.lr_links_approx on the layout scaled to 2400 SNPs (above the 2000 its searchsorted fast path needs) against orc.lr_links_approx, at sr_dist on
    and beside the grid, 0, just below g / 2 and g / 2 (no fast path there); then the same positions with the SNPs that are NOT sampled permuted: the
    list no longer ascends, the slow path runs, and the sampled SNPs and the positions as a set are the same — so must the count be."""
    from ldweaver_amd import rcompat
    n = 2400
    POS = _positions(n, g)
    idx = rcompat.r_sample(1988, n, int(round(n * 0.1))) - 1
    rest = np.setdiff1d(np.arange(n), idx)
    perm = np.arange(n)
    perm[rest] = np.random.default_rng(20274).permutation(rest)
    POSp = POS[perm]
    assert np.array_equal(POSp[idx], POS[idx]) and np.any(np.diff(POSp) < 0) and np.array_equal(np.sort(POSp), POS)
    for sr_dist in (2000.0, 2001.0, 0.0, 119999.5, 120000.0):
        want = orc.lr_links_approx(POS, g, sr_dist)
        assert MIH.lr_links_approx(POS, g, sr_dist) == want, (g, sr_dist)
        assert MIH.lr_links_approx(POSp, g, sr_dist) == want, (g, sr_dist, "slow path")
