"""The per-slot device buffers of a block's launch chain (ldweaver_amd/csrc/ldw_slots.h) when they have to GROW where they are used (pytest -m gpu):
a context whose ldw_ctx_reserve sized them for blocks of 64 SNPs runs blocks of 500 and of 2048 — units, packs, pair lists, bins and the maybe list's
extracts are all reallocated inside the pass, while other slots are in flight — and then a smaller problem.  Link tables against the plain path, bit for
bit.  (The inputs were checked with the numpy oracle beforehand: 29 370 short-range and 4 542 long-range rows at blocks of 500, 122 250 and 75 590 at 2048.)"""
import os

import numpy as np
import pytest

from ldweaver_amd import _lib as L
from ldweaver_amd import mi as MIH
from ldweaver_amd.engine import Engine
from ldweaver_amd.synth import synth_alignment

pytestmark = pytest.mark.gpu

SR_DIST = 2000.0


def clustered_problem(Ls, N, B, seed):
    """A multi-allelic synthetic alignment (third alleles, gaps) whose positions come in clusters of B SNPs, 100 bp apart within a cluster and a million
    between clusters: with blocks of B and sr_dist = 2000 every diagonal block holds short-range pairs and every off-diagonal block is long-range only."""
    syn = synth_alignment(Ls, N, seed=seed)
    k = np.arange(Ls)
    POS = ((k // B) * 1_000_000 + (k % B) * 100 + 1).astype(np.int32)
    g = float((Ls + B - 1) // B * 1_000_000 + 1_000_000)
    return dict(states=syn["states"], POS=POS, paint=syn["paint"], g=g, blocks=MIH.make_blocks(Ls, B), retain=0.004 * Ls * Ls / 2)


def _load(eng, d, max_blk_sz=10000):
    """max_blk_sz: what the context's first set_alignment hands to ldw_ctx_reserve (the engine reserves once per context)."""
    eng.set_engine(L.ENGINE_MFMA)
    eng.set_alignment(d["states"], max_blk_sz)
    cnt = eng.state_counts()
    uqe = (cnt > 0).T.astype(np.float64)
    eng.set_weights(eng.hamming_weights(int(d["states"].shape[0] * 0.1)))
    eng.set_snp_meta(uqe.sum(axis=1), uqe, d["POS"], d["paint"], d["g"])
    d["approx"] = MIH.lr_links_approx(d["POS"], d["g"], SR_DIST)


def _run(eng, d, plain, cold):
    eng.set_mixed(not plain)
    eng.set_screen(0 if plain else 1)
    eng.set_path(1 if plain else 0)
    if cold:
        eng.reset_speculation()
    eng.mi_all_pairs(d["blocks"], SR_DIST, d["retain"], d["approx"])
    return eng.links(0), eng.links(1)


def _same(x, y, what):
    for which in (0, 1):
        assert len(x[which][2]) > 0, (what, which)
        for a, b in zip(x[which], y[which]):
            assert np.array_equal(a, b), (what, which)


# (Ls, N, B, a span can form).  A block joins a span only from 2048 SNPs a side on (span_candidate, ldw_pass_plan.h): the blocks of 500 exercise the growth
# of every buffer of ordinary items, the blocks of 2048 that of a span's.
@pytest.mark.parametrize("Ls,N,B,spans", [(1500, 2100, 500, False), (6144, 2100, 2048, True)])
def test_slot_buffers_grow_where_they_are_used(Ls, N, B, spans):
    """Ls SNPs x 2100 sequences (KW = 34: the maybe list is on) in three clusters of B — three diagonal blocks with short-range pairs, three long-range-only
    blocks of which two may form a span — on a context that reserved for blocks of 64 (ldw_slot_report shows the buffers growing inside the passes).
    Default path == plain path, cold and warm, with the queue placement of short alignments and with that of long ones (LDW_QUEUE_SWAP_KW = 1); the
    maybe list handed entries over, nothing overflowed, the approximate path took blocks and, where blocks are large enough to join one, a span ran.
    Then N = 130 on the same context == a fresh context."""
    big = clustered_problem(Ls, N, B, seed=61)
    small = clustered_problem(700, 130, 300, seed=62)
    assert os.environ.get("LDW_QUEUE_SWAP_KW") is None
    with Engine(0) as eng:
        _load(eng, big, 64)          # the context's one reservation: slot buffers for blocks of 64 in spans of 8
        plain = _run(eng, big, True, True)
        p0, s0, o0, b0 = eng.path_report(), eng.span_report(), eng.overflow_report(), eng.slot_report()
        try:
            for swap in (None, "1"):
                if swap:
                    os.environ["LDW_QUEUE_SWAP_KW"] = swap
                _same(plain, _run(eng, big, False, True), ("cold", swap))
                _same(plain, _run(eng, big, False, False), ("warm", swap))
        finally:
            os.environ.pop("LDW_QUEUE_SWAP_KW", None)
        p1, s1, o1, b1 = eng.path_report(), eng.span_report(), eng.overflow_report(), eng.slot_report()
        print(f"blocks of {B}: sr rows {len(plain[0][2])} lr rows {len(plain[1][2])}; path {p0} -> {p1}; spans {s0} -> {s1}; overflow {o0} -> {o1}; slot buffers {b0} -> {b1}")
        # the buffers did grow inside the passes: an item of 500 x 500 has more from-tiles (>= 8 against 7), units and pair-list entries than the reserved
        # 64 x 512 (its row arrays are shorter: the bins need not grow), a span of 2048 x 4096 is larger in every dimension
        assert b0["units"] > 0 and b1["grown"] >= b0["grown"] + 4, (b0, b1)
        for k in ("units", "packs", "pairs", "mini") + (("bins",) if spans else ()):
            assert b1[k] > b0[k], (k, b0, b1)
        if spans:
            assert s1["spans"] > s0["spans"] and s1["blocks"] - s0["blocks"] >= 2, (s0, s1)
        assert o1["maybe_entries"] > o0["maybe_entries"], (o0, o1)
        assert o1["pair_list"] == o0["pair_list"] and o1["maybe_list"] == o0["maybe_list"] and not o1["maybe_off"], (o0, o1)
        assert p1["apx_blocks"] > p0["apx_blocks"], (p0, p1)
        # a smaller problem on the context that has run the larger one
        _load(eng, small)
        used = [_run(eng, small, False, True), _run(eng, small, False, False)]
    with Engine(0) as fresh:
        _load(fresh, small)
        _same(_run(fresh, small, True, True), used[0], "small problem, used context, cold")
        _same(_run(fresh, small, False, True), used[0], "small problem, fresh against used, cold")
        _same(_run(fresh, small, False, False), used[1], "small problem, fresh against used, warm")
