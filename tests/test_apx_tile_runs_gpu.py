"""GPU: the approximate GEMM's list launch, in which a wave walks a RUN of the live-tile list (pytest -m gpu).

gemm_apx_kernel stages its tables once per workgroup; wave w of a grid of g workgroups then computes the tiles w, w + 4 g, ... of the list and asks for
the first panel pieces of its next tile before the epilogue of the current one.  None of that may change a value:

  * through ldw_debug_apx_gemm_list (a list of every tile, a forced grid, no table test) the int32 sums equal those of the 2-D launch of
    ldw_debug_apx_gemm entry for entry, and both lie within the truncation bound of the exact integer sums S' (BOUNDS.md 2), for 1, 2, 3, 4, 6 and 9
    tiles (nrt in {100, 128, 129, 384} x nrf in {40, 64, 65, 192}: tiles are 128 to-rows x 64 from-rows, so no pair of these sizes gives 5 — with one
    workgroup 6 and 9 tiles make waves walk two and three tiles next to waves that walk one fewer), grids of one workgroup (every wave walks), two,
    and more workgroups than tiles (the surplus leaves unstaged), unit weights and Hamming weights with exponent transitions, K loops of 2 and 6
    macro steps;
  * end to end the link tables of the default path under LDW_APX_GRID_WGS = 1, = 3, unset, and under LDW_NO_APX_RUNS=1 (one tile per wave, the
    launch as it was) equal the plain path's (5-limb GEMM, fp64 MI of every pair) bit for bit, cold and warm, with no screen violation in verify
    mode, also on a context that has just run a larger problem."""
import os

import numpy as np
import pytest

from ldweaver_amd import _lib as L
from ldweaver_amd import mi as MIH
from ldweaver_amd.engine import Engine
from ldweaver_amd.synth import synth_alignment

pytestmark = pytest.mark.gpu

NRT, NRF = (100, 128, 129, 384), (40, 64, 65, 192)
SR_DIST = 20000.0
RETAIN = 0.004   # long-range links kept, as a share of all: below 0.007 the pass speculates on its thresholds, which is what opens the approximate path


def _tiles(nrt, nrf):
    return -(-nrt // 128) * -(-nrf // 64)


def test_the_shapes_cover_the_tile_counts():
    assert sorted({_tiles(a, b) for a in NRT for b in NRF}) == [1, 2, 3, 4, 6, 9]


# ------------------------------------------------------------------------------------------------
# the kernel through its two launch forms
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,seed", [("unit", 200, 41), ("hamming", 200, 42), ("unit", 700, 43), ("hamming", 700, 44)])
def test_list_launch_equals_the_2d_launch_and_the_exact_sums(engine, kind, N, seed):
    syn = synth_alignment(500, N, seed=seed)
    st = np.asarray(syn["states"])
    engine.set_engine(L.ENGINE_MFMA)
    engine.set_alignment(st)
    hdw = engine.hamming_weights(50) if kind == "hamming" else np.ones(N)
    uqe = (engine.state_counts() > 0).T.astype(np.float64)
    engine.set_weights(hdw)
    engine.set_snp_meta(uqe.sum(axis=1), uqe, syn["POS"], syn["paint"], float(syn["g"]))
    par, V, Va = engine.debug_apx_params()
    P = dict(zip(Engine.APX_PARAM_NAMES, par))
    assert int(P["flags"]) & 1, engine.path_report()["apx_gate"]
    el = int(P["e_last"])
    if kind == "unit":
        assert el == 0 and P["lost_units"] == 0        # no transition: nothing is truncated
    else:
        assert el > 0 and P["lost_units"] > 0          # lost_units adds one term per exponent transition: there is at least one

    # the bits of every indicator row (+ the all-zero padding row R) and the exact integer sums of the dual-digit weights, once
    row0, meta = engine.debug_rows()
    R = int(row0[-1])
    bits = np.zeros((R + 1, N), dtype=bool)
    for a in range(len(st)):
        m = int(meta[a])
        for i in range(m & 7):
            bits[int(row0[a]) + i] = st[a] == ((m >> (8 + 3 * i)) & 7)
    assert R >= 400
    rng = np.random.default_rng(seed)
    wb = bits.astype(np.float64) * Va.astype(np.float64)
    for nrt in NRT:
        for nrf in NRF:
            rt = np.append(rng.choice(R, nrt - 1, replace=False), R).astype(np.int32)     # (the padding row: no sequence)
            rf = np.append(rng.choice(R, nrf - 1, replace=False), R).astype(np.int32)
            S = wb[rt] @ bits[rf].astype(np.float64).T                                     # exact: integers below 2^52
            G = engine.debug_apx_gemm(rt, rf)
            lost = S - G.astype(np.int64) * 2.0 ** el
            assert lost.min() >= 0.0 and lost.max() <= P["lost_units"] * 2.0 ** el, (nrt, nrf, lost.min(), lost.max())
            assert np.all(G[-1] == 0) and np.all(G[:, -1] == 0)
            tiles = _tiles(nrt, nrf)
            for grid in (1, 2, tiles // 4 + 3):
                Gl = engine.debug_apx_gemm(rt, rf, grid_wgs=grid)
                assert np.array_equal(Gl, G), (kind, N, nrt, nrf, tiles, grid, int((Gl != G).sum()))
    print(f"{kind} N {N}: e_last {el}, lost units bound {P['lost_units']:.3f}, {len(NRT) * len(NRF)} shapes x 3 grids equal the 2-D launch")


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
def _load(eng, Ls, N, seed):
    syn = synth_alignment(Ls, N, seed=seed)
    eng.set_engine(L.ENGINE_MFMA)
    eng.set_alignment(np.asarray(syn["states"]))
    uqe = (eng.state_counts() > 0).T.astype(np.float64)
    eng.set_weights(eng.hamming_weights(int(Ls * 0.1)))
    POS, g = syn["POS"], float(syn["g"])
    eng.set_snp_meta(uqe.sum(axis=1), uqe, POS, syn["paint"], g)
    return POS, g


def _same(x, y, what):
    for which in (0, 1):
        assert len(x[which][2]) == len(y[which][2]), (what, which, len(x[which][2]), len(y[which][2]))
        for a, b in zip(x[which][:2], y[which][:2]):
            assert np.array_equal(a, b), (what, which)
        assert np.array_equal(x[which][2].view(np.uint64), y[which][2].view(np.uint64)), (what, which, "MI bits")


class _Env:
    """The two switches of the list launch, read by the library per call."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k in ("LDW_APX_GRID_WGS", "LDW_NO_APX_RUNS"):
            assert k not in os.environ, k
        os.environ.update(self.kw)

    def __exit__(self, *exc):
        for k in self.kw:
            os.environ.pop(k)


FORMS = [("grid 1", dict(LDW_APX_GRID_WGS="1")), ("grid 3", dict(LDW_APX_GRID_WGS="3")), ("default grid", {}), ("one tile per wave", dict(LDW_NO_APX_RUNS="1"))]


def _forms_equal_plain(eng, Ls, N, blk, seed, forms=FORMS, warm=True, want_spans=False):
    POS, g = _load(eng, Ls, N, seed)
    blocks = MIH.make_blocks(Ls, blk)
    approx = MIH.lr_links_approx(POS, g, SR_DIST)

    def run(cold):
        if cold:
            eng.reset_speculation()
        eng.mi_all_pairs(blocks, SR_DIST, RETAIN * approx, approx)
        return eng.links(0), eng.links(1)

    try:
        eng.set_mixed(False); eng.set_screen(0); eng.set_path(1)
        plain = run(True)
        assert len(plain[0][2]) > 0 and len(plain[1][2]) > 0
        eng.set_mixed(True); eng.set_screen(1); eng.set_path(0)
        seen = {}
        for tag, env in forms:
            with _Env(**env):
                c0, p0, o0, s0 = eng.counters(), eng.path_report(), eng.overflow_report(), eng.span_report()
                _same(plain, run(True), (tag, "cold"))
                if warm:
                    _same(plain, run(False), (tag, "warm"))
                c1, p1, o1, s1 = eng.counters(), eng.path_report(), eng.overflow_report(), eng.span_report()
                # the approximate path really ran (else the forms are one and the same code)
                assert p1["apx_blocks"] - p0["apx_blocks"] > 0, (tag, p1["apx_gate"])
                if want_spans:
                    assert s1["spans"] - s0["spans"] >= 1, (tag, s0, s1)
                seen[tag] = (c1["spec_misses"] - c0["spec_misses"], {k: o1[k] - o0[k] for k in o1 if not isinstance(o1[k], bool)})
                eng.set_screen(2)      # verify mode: every pair the screen dismisses is evaluated too
                v0 = eng.counters()["screen_violations"]
                _same(plain, run(True), (tag, "verify"))
                assert eng.counters()["screen_violations"] - v0 == 0, tag
                eng.set_screen(1)
        first = seen[forms[0][0]]
        for tag, _ in forms:
            assert seen[tag] == first, (tag, seen)
    finally:
        eng.set_mixed(True); eng.set_screen(1); eng.set_path(0)


def test_every_form_of_the_list_launch_gives_the_plain_path_tables():
    """1500 SNPs x 300 sequences in blocks of 500: diagonal blocks (the 2-D launch, its workgroups above the diagonal leaving unstaged), blocks with a
    short-range corner and long-range-only blocks (the list launch).  Spans need blocks of at least 2048 SNPs: the next test has one."""
    with Engine(0) as eng:
        _forms_equal_plain(eng, 1500, 300, 500, seed=71)


def test_a_span_walked_in_runs_gives_the_plain_path_tables():
    """10240 SNPs x 300 sequences in five blocks of 2048: the first block row holds a span of two long-range-only blocks (its last block is a corner
    block again: the genome is a circle), whose list launch is the longest
    (blocks this small are not probed, so the cold pass has no threshold guess to plan spans on: the warm pass has)."""
    with Engine(0) as eng:
        _forms_equal_plain(eng, 10240, 300, 2048, seed=72, forms=[FORMS[1], FORMS[2]], want_spans=True)


def test_runs_after_a_larger_problem_on_the_same_context():
    """A stale count of live tiles (or anything else a larger block left in the slot) would send a wave of the smaller problem beyond its own list."""
    with Engine(0) as eng:
        POS, g = _load(eng, 3000, 520, seed=73)
        with _Env(LDW_APX_GRID_WGS="2"):
            approx = MIH.lr_links_approx(POS, g, SR_DIST)
            eng.mi_all_pairs(MIH.make_blocks(3000, 1000), SR_DIST, RETAIN * approx, approx)
        assert eng.path_report()["apx_blocks"] > 0
        _forms_equal_plain(eng, 1500, 300, 500, seed=71, forms=FORMS[:3], warm=False)
