"""The failure edges of the item loop of ldw_mi_all_pairs (csrc/ldw_mi_pass.inc; pytest -m gpu): a pass whose block list holds ONE bad descriptor
(te = L + 1) at block 0 (nothing submitted yet), at the last block, and at a block the good plan holds in the middle of a span — each without and with
lr_links.tsv streaming.  Every case: LDW_ERR_ARG with "outside 1..", the streamed file is byte for byte the head of the complete file for the blocks
in front of the bad one, and the good list run at once on the same context gives the tables and block statistics it gave before.

16 384 SNPs x 512 sequences in 8 x 8 blocks of 2048 — the smallest square block a span takes (span_candidate, ldw_pass_plan.h) — 36 block pairs.
Positions 100 apart on a circle of 100 L + 100 with sr_dist = 20 000 (200 SNPs): 2 sr_dist < g, neighbouring blocks and the pair that closes the
circle hold short-range corners, every other off-diagonal block is long-range only: the rows hold spans of 5, 5, 4, 3 and 2 blocks (blocks 2..6 of
row 0 are one).  No block reaches the cold-start probe's minimum, so the spans form on the guesses an earlier pass left: the passes here run warm."""
import numpy as np
import pytest

from ldweaver_amd import _lib as L
from ldweaver_amd import mi as MIH
from ldweaver_amd.engine import Engine
from ldweaver_amd.synth import synth_alignment

pytestmark = pytest.mark.gpu

LS, N, B = 16_384, 512, 2_048
SR_DIST = 20_000.0


def test_one_bad_block_at_the_edges_of_the_item_loop(tmp_path):
    with Engine(0) as engine:   # (a context of its own: the library's default switches, nobody else's guesses)
        _edges(engine, tmp_path)


def _edges(engine, tmp_path):
    syn = synth_alignment(LS, N, seed=1988, device="cuda", as_numpy=False)
    POS = (100 * np.arange(LS) + 1).astype(np.int32)
    g = float(100 * LS + 100)
    engine.set_engine(L.ENGINE_MFMA)
    engine.set_alignment(syn["states"])
    cnt = engine.state_counts()
    uqe = (cnt > 0).T.astype(np.float64)
    engine.set_weights(engine.hamming_weights(int(LS * 0.1)))
    engine.set_snp_meta(uqe.sum(axis=1), uqe, POS, syn["paint"], g)
    blocks = MIH.make_blocks(LS, B)
    assert len(blocks) == 36
    kw = dict(sr_dist=SR_DIST, lr_retain_links=2e5, lr_links_approx=MIH.lr_links_approx(POS, g, SR_DIST))

    def result():
        return engine.links(0), engine.links(1), engine.block_stats()

    def same(x, y, what):
        for which in (0, 1):
            for a, b in zip(x[which], y[which]):
                assert np.array_equal(a, b), (what, which)
        for k in ("n_lr_total", "n_lr_kept", "n_sr", "disc_thresh"):
            assert np.array_equal(x[2][k], y[2][k]), (what, k)

    engine.set_span(True, 8)
    engine.reset_speculation()
    engine.mi_all_pairs(blocks, **kw)           # cold: leaves the guesses
    cold = result()
    s0 = engine.span_report()
    engine.mi_all_pairs(blocks, **kw)           # warm: plans spans
    s1 = engine.span_report()
    # every long-range-only block of the five rows ran in a span: block 4 sits in the middle of the first one (blocks 2..6)
    assert (s1["spans"] - s0["spans"], s1["blocks"] - s0["blocks"]) == (5, 19), (s0, s1)
    want = result()
    same(cold, want, "cold against warm")
    kept = want[2]["n_lr_kept"]
    assert len(want[0][2]) > 100_000 and int(kept.sum()) == len(want[1][2]) > 50_000 and np.all(kept > 0)

    # the complete file, streamed; what it starts with in front of its first row (nothing, today) belongs to every head
    whole = tmp_path / "whole.tsv"
    engine.lr_stream_begin(str(whole), append=False)
    engine.mi_all_pairs(blocks, **kw)
    rows, nbytes, nblk = engine.lr_stream_end()
    assert (rows, nblk) == (int(kept.sum()), len(blocks))
    same(result(), want, "streamed")
    ref = whole.read_bytes()
    assert len(ref) == nbytes
    lines = ref.split(b"\n")
    assert lines[-1] == b"" and len(lines) - 1 >= rows
    n_head = len(lines) - 1 - rows

    for k in (0, len(blocks) - 1, 4):
        bad = blocks.copy()
        bad[k, 3] = LS + 1
        want_rows = int(kept[:k].sum())
        for stream in (False, True):
            f = tmp_path / f"fail_{k}.tsv"
            if stream:
                engine.lr_stream_begin(str(f), append=False)
            with pytest.raises(L.LdwError) as ei:
                engine.mi_all_pairs(bad, **kw)
            assert ei.value.code == L.LDW_ERR_ARG and "outside 1.." in str(ei.value), (k, stream, str(ei.value))
            assert f"block {k} = " in str(ei.value), (k, stream, str(ei.value))
            if stream:
                rows, nbytes, nblk = engine.lr_stream_end()
                assert (nblk, rows) == (k, want_rows), (k, nblk, rows, want_rows)
                assert f.read_bytes() == b"".join(l + b"\n" for l in lines[:n_head + want_rows]), k
            s2 = engine.span_report()
            engine.mi_all_pairs(blocks, **kw)
            same(result(), want, ("good list after block", k, "streaming" if stream else "plain"))
            s3 = engine.span_report()
            assert (s3["spans"] - s2["spans"], s3["blocks"] - s2["blocks"]) == (5, 19), (k, stream, s2, s3)
