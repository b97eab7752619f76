"""GPU: what the FUSED approximate GEMM does with the values it accumulates, entry by entry (pytest -m gpu).

The value gemm_apx_kernel accumulates is tested elsewhere (tests/test_apx_tile_runs_gpu.py, BOUNDS.md 2-3).  In the product every launch of it is fused: the
live-tile pass k_apx_live_tiles decides which 128 x 64 wave tiles are computed at all (pruning rules (a) and (b)), and apx_gemm_epilogue tests every region of
32 to-rows x 64 from-rows against the threshold table — clean and not stored, at most APX_MAYBE_MAX failing entries handed to the maybe list, or stored.
ldw_debug_apx_gemm_fused runs exactly those launches on caller-made bins, flags, table, mask and capacity over buffers filled with a pattern; every flag
byte, every int32 of G', the live-tile list, the pruned count and the maybe list are compared with the plain model of tests/apx_fused_ref.py.  Everything is
an integer: there is no tolerance.

The accumulators the model starts from are the exact counts (unit weights) or the matrix of the no-table launch ldw_debug_apx_gemm on the same rows, itself
held against the exact sums S' first: the epilogue's input is pinned by a launch that does not run the epilogue.  The cases are those of
tests/apx_fused_cases.py (see tests/test_apx_fused_cases_host.py for what they must hold), rebuilt over each weighting's accumulators and checked again for
their situations: 25 shapes of 2 to 16 wave tiles, three weightings (unit; Hamming weights with exponent transitions; five orders of magnitude, the
kernel's FINE instantiation), K loops of 2 and 6 macro steps, and five launch forms — the 2-D launch and the list launch behind the live-tile pass with one
workgroup (every wave walks a run of up to four tiles), two, more workgroups than tiles, and the default path's grid."""
import time

import numpy as np
import pytest

import apx_fused_cases as CS
import apx_fused_ref as REF
from ldweaver_amd import _lib as L
from ldweaver_amd.engine import Engine
from ldweaver_amd.synth import synth_alignment

pytestmark = pytest.mark.gpu

FILL8, FILL32 = Engine.APX_FUSED_FILL, Engine.APX_FUSED_FILL32
FILLU32 = int(np.frombuffer(bytes([FILL8] * 4), dtype=np.uint32)[0])
LOADS = [("unit", 200, 41), ("hamming", 200, 42), ("wide", 200, 45), ("unit", 700, 43), ("hamming", 700, 44), ("wide", 700, 46)]
_loaded = {}        # the one weighting the session's engine holds now: its key and its cases


def _load(engine, kind, N, seed):
    if _loaded.get("key") == (kind, N, seed):
        return _loaded
    syn = synth_alignment(500, N, seed=seed)
    st = np.asarray(syn["states"])
    engine.set_engine(L.ENGINE_MFMA)
    engine.set_alignment(st)
    if kind == "hamming":
        hdw = engine.hamming_weights(50)
    elif kind == "wide":            # five orders of magnitude (tests/test_bounds.py): one exponent per 32 positions
        hdw = 10.0 ** np.random.default_rng(seed).uniform(-5.0, 0.0, N)
    else:
        hdw = np.ones(N)
    uqe = (engine.state_counts() > 0).T.astype(np.float64)
    engine.set_weights(hdw)
    engine.set_snp_meta(uqe.sum(axis=1), uqe, syn["POS"], syn["paint"], float(syn["g"]))
    par, V, Va = engine.debug_apx_params()
    P = dict(zip(Engine.APX_PARAM_NAMES, par))
    flags, el = int(P["flags"]), int(P["e_last"])
    assert flags & 1, engine.path_report()["apx_gate"]
    # the template each weighting is there for (a case must not silently run the other one)
    if kind == "unit":
        assert el == 0 and P["lost_units"] == 0 and not flags & 2
    elif kind == "hamming":
        assert el > 0 and P["lost_units"] > 0 and not flags & 2          # at least one exponent transition, one exponent per macro step
    else:
        assert flags & 2 and P["lost_units"] > 0                          # gemm_apx_kernel<.., FINE = true>
    row0, meta = engine.debug_rows()
    R = int(row0[-1])
    bits = np.zeros((R + 1, N), dtype=bool)
    for a in range(len(st)):
        m = int(meta[a])
        for i in range(m & 7):
            bits[int(row0[a]) + i] = st[a] == ((m >> (8 + 3 * i)) & 7)
    wb = bits.astype(np.float64) * Va.astype(np.float64)

    def acc_of(rt, rf):
        if kind == "unit":
            return bits[rt].astype(np.int64) @ bits[rf].astype(np.int64).T
        G = engine.debug_apx_gemm(rt, rf)                                  # the 2-D launch without a table: no epilogue test runs
        S = wb[rt] @ bits[rf].astype(np.float64).T                         # exact: integers below 2^52
        lost = S - G.astype(np.int64) * 2.0 ** el
        assert lost.min() >= 0.0 and lost.max() <= P["lost_units"] * 2.0 ** el, (kind, N, len(rt), len(rf), lost.min(), lost.max())
        return G.astype(np.int64)

    cases = CS.make_cases(R, acc_of, seed)
    _loaded.clear()
    _loaded.update(key=(kind, N, seed), cases=cases)
    return _loaded


def _forms(c):
    tiles = -(-c["nrt"] // 128) * 2 * -(-c["nrf"] // 128)
    return [(False, 0)] + [(True, g) for g in (1, 2, tiles // 4 + 3, 0)]


def _check(c, prune, grid, out):
    """One launch against the model: every output buffer, whole."""
    E = CS.expect(c, prune)
    what = (c["name"], c["nrt"], c["nrf"], "prune" if prune else "2-D", grid)
    acc = c["acc"]
    RTpad, RFpad = acc.shape
    ntx = RFpad // 64
    stored = REF.stored_entries(E, acc.shape)
    G = out["G"]
    for g, x in zip(*np.nonzero(E.stored)):             # (print the figure before the assertion: which region, how many entries)
        rs, cs = slice(32 * g, 32 * g + 32), slice(64 * x, 64 * x + 64)
        assert np.array_equal(G[rs, cs], acc[rs, cs]), (what, "stored region", int(g), int(x), int((G[rs, cs] != acc[rs, cs]).sum()))
    assert np.all(G[~stored] == FILL32), (what, "written outside the stored regions", int((G[~stored] != FILL32).sum()))
    want_flags = np.where(E.clean == REF.UNWRITTEN, FILL8, E.clean).astype(np.uint8)
    assert np.array_equal(out["clean"], want_flags), (what, "clean flags", out["clean"].tolist(), want_flags.tolist())
    tiles = out["tiles"]
    if prune:
        n = out["n_live"]
        assert n == len(E.live) and out["pruned"] == E.pruned, (what, "live / pruned", n, len(E.live), out["pruned"], E.pruned)
        assert {int(t) for t in tiles[:n]} == {y * ntx + x for y, x in E.live}, (what, "live-tile set", tiles[:n].tolist())
        tys = [int(t) // ntx for t in tiles[:n]]
        runs = [y for k, y in enumerate(tys) if k == 0 or tys[k - 1] != y]
        assert len(runs) == len(set(runs)), (what, "the tiles of one ty are not consecutive", tiles[:n].tolist())
        assert all(tiles[k] < tiles[k + 1] for k in range(n - 1) if tys[k] == tys[k + 1]), (what, "tx does not ascend", tiles[:n].tolist())
        assert np.all(tiles[n:] == FILLU32), (what, "list written beyond n_live")
    else:
        assert out["n_live"] == 0 and out["pruned"] == 0 and np.all(tiles == FILLU32), what
    cap = c["maybe_cap"]
    assert out["maybe_n"] == E.maybe_n, (what, "maybe_n", out["maybe_n"], E.maybe_n)
    assert out["beyond_cap"] == 0, (what, "bytes written behind the capacity of the maybe list", out["beyond_cap"])
    if cap > 0:
        n = min(E.maybe_n, cap)
        got = sorted(tuple(int(v) for v in row) for row in out["maybe"][:n])
        assert np.all(out["maybe"][n:] == FILL32), (what, "maybe list written beyond", n)
        if E.maybe_n <= cap:
            assert got == E.maybe, (what, "maybe entries", [e for e in got if e not in E.maybe][:5], [e for e in E.maybe if e not in got][:5])
        else:                           # an overflowing list: which entries fit depends on the order of the waves, not what they are
            assert len(set(got)) == n and set(got) <= set(E.maybe), (what, "maybe entries of the overflowing list", [e for e in got if e not in E.maybe][:5])
    return E


@pytest.mark.parametrize("nrt", CS.NRT)
@pytest.mark.parametrize("kind,N,seed", LOADS)
def test_fused_launches_equal_the_model(engine, kind, N, seed, nrt):
    S = _load(engine, kind, N, seed)
    t0 = time.perf_counter()
    stats0, prune0 = engine.gemm_stats(), engine.prune_report()
    launches = 0
    for c in S["cases"]:
        if c["nrt"] != nrt:
            continue
        first = {}
        for prune, grid in _forms(c):
            out = engine.debug_apx_gemm_fused(c["rows_t"], c["rows_f"], c["bin_t"], c["bin_f"], c["tab"], c["rflag_t"], c["rflag_f"], c["sr_mask"], c["lower_only"], prune, grid,
                                              c["maybe_cap"])
            launches += 1
            E = _check(c, prune, grid, out)
            # every launch form gives the same flags, stores and maybe multiset as every other (the 2-D launch is never handed the row flags: it
            # equals the others where rule (b) pruned nothing)
            same = "all" if CS.expect(c, True).pruned_b == 0 else ("list" if prune else "2-D")
            mb = sorted(map(tuple, out["maybe"][:min(out["maybe_n"], max(c["maybe_cap"], 0))].tolist()))
            if same in first:
                G0, clean0, mb0 = first[same]
                assert np.array_equal(out["G"], G0) and np.array_equal(out["clean"], clean0), (c["name"], nrt, c["nrf"], prune, grid)
                if E.maybe_n <= max(c["maybe_cap"], 0):
                    assert mb == mb0, (c["name"], nrt, c["nrf"], prune, grid)
            else:
                first[same] = (out["G"], out["clean"], mb)
    assert engine.gemm_stats() == stats0 and engine.prune_report() == prune0
    print(f"{kind} N {N} nrt {nrt}: {launches} fused launches equal the model, {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("kind,N,seed", LOADS)
def test_the_cases_hold_their_situations_on_these_accumulators(engine, kind, N, seed):
    """The conditions of tests/test_apx_fused_cases_host.py, on the accumulators this weighting really gives (the two that ask for NEIGHBOURING integers in
    one row of a region are a matter of the exact counts: weighted sums are sparse)."""
    S = _load(engine, kind, N, seed)
    seen = set().union(*(CS.situations(c) for c in S["cases"]))
    for name in CS.REQUIRED:
        if kind != "unit" and name in ("Lq + 1 present and passes", "Hq - 1 present and passes"):
            continue
        assert name in seen, f"{kind} N {N}: no case holds: {name}"


def test_refusals_launch_nothing_and_write_nothing(engine):
    S = _load(engine, *LOADS[0])
    c = next(c for c in S["cases"] if c["name"] == "rule_b" and c["nrt"] == 129 and c["nrf"] == 65)
    R = int(engine.debug_rows()[0][-1])
    stats0, prune0 = engine.gemm_stats(), engine.prune_report()

    def refused(code, maybe_cap=64, **kw):
        a = dict(rows_t=c["rows_t"], rows_f=c["rows_f"], bin_t=c["bin_t"], bin_f=c["bin_f"], tab=c["tab"], rflag_t=c["rflag_t"], rflag_f=c["rflag_f"], prune=True, grid_wgs=1)
        a.update(kw)
        out = dict(G=np.full((256, 128), 77, dtype=np.int32), clean=np.full((8, 2), 77, dtype=np.uint8), tiles=np.full(4, 77, dtype=np.uint32),
                   maybe=np.full((max(maybe_cap, 1), 3), 77, dtype=np.int32))
        with pytest.raises(L.LdwError) as e:
            engine.debug_apx_gemm_fused(maybe_cap=maybe_cap, out=out, **a)
        assert e.value.code == code, (kw, e.value)
        assert all(np.all(v == 77) for v in out.values()), kw

    def with_entry(a, k, v):
        b = np.array(a).copy()
        b[k] = v
        return b

    refused(L.LDW_ERR_ARG, rows_t=with_entry(c["rows_t"], 5, R + 1))
    refused(L.LDW_ERR_ARG, rows_f=with_entry(c["rows_f"], 64, -1))
    refused(L.LDW_ERR_ARG, bin_t=with_entry(c["bin_t"], 128, 64))
    refused(L.LDW_ERR_ARG, bin_f=with_entry(c["bin_f"], 0, 254))
    refused(L.LDW_ERR_ARG, prune=False, grid_wgs=1)
    refused(L.LDW_ERR_ARG, grid_wgs=-1)
    refused(L.LDW_ERR_ARG, grid_wgs=65537)
    refused(L.LDW_ERR_ARG, maybe_cap=0)
    refused(L.LDW_ERR_ARG, maybe_cap=-2)
    refused(L.LDW_ERR_ARG, maybe_cap=(1 << 20) + 1)
    refused(L.LDW_ERR_ARG, rflag_f=None)
    refused(L.LDW_ERR_ARG, rflag_t=None)
    assert engine.gemm_stats() == stats0 and engine.prune_report() == prune0
    # the same call goes through once nothing is wrong with it, at the largest legal grid and capacity
    out = engine.debug_apx_gemm_fused(c["rows_t"], c["rows_f"], c["bin_t"], c["bin_f"], c["tab"], c["rflag_t"], c["rflag_f"], prune=True, grid_wgs=65536, maybe_cap=1 << 20)
    big = dict(c, maybe_cap=1 << 20)
    big["expect"] = {}
    _check(big, True, 65536, out)
    assert engine.gemm_stats() == stats0 and engine.prune_report() == prune0
    # a context whose weights do not allow the approximate path (it has none)
    with Engine(0) as eng:
        syn = synth_alignment(120, 64, seed=3)
        eng.set_alignment(np.asarray(syn["states"]))
        with pytest.raises(L.LdwError) as e:        # no weights at all
            eng.debug_apx_gemm_fused(c["rows_t"][:4] * 0, c["rows_f"][:4] * 0, c["bin_t"][:4], c["bin_f"][:4], c["tab"])
        assert e.value.code == L.LDW_ERR_STATE, e.value
