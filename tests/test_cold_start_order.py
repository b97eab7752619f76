"""The start of a pass (ldw_mi_all_pairs): the plan is made before the cold-start probes are queued, the first item is submitted as soon as the
probe of ITS kind is back, the other probe is collected behind it.  None of that may decide a row: for block lists that take every way through
that start-up, the short- and long-range tables of the default path equal the plain path's (set_path(1), set_screen(0), set_mixed(False)) row
for row, cold (speculation state reset) and warm, on one context reused across the cases."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ldweaver_amd import mi as MIH
from ldweaver_amd.dist import deal_blocks
from ldweaver_amd.engine import Engine
from ldweaver_amd.synth import synth_alignment

pytestmark = pytest.mark.gpu

LS, N, B = 40_000, 2_000, 8_000   # diagonal blocks of 32 M pairs, off-diagonal ones of 64 M: both kinds are probed (16 M pairs at least)
SR_DIST, RETAIN = 20000.0, 1e6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Ctx:
    def __init__(self):
        self.eng = Engine(0)
        syn = synth_alignment(LS, N, seed=1988, device="cuda", as_numpy=False)
        e = self.eng
        e.set_alignment(syn["states"])
        cnt = e.state_counts()
        uqe = (cnt > 0).T.astype(np.float64)
        self.hdw = e.hamming_weights(int(LS * 0.1))
        self.hdw_other = e.hamming_weights(int(LS * 0.2))
        e.set_weights(self.hdw)
        self.POS, self.g = syn["POS"], float(syn["g"])
        e.set_snp_meta(uqe.sum(axis=1), uqe, self.POS, syn["paint"], self.g)
        self.approx = MIH.lr_links_approx(self.POS, self.g, SR_DIST)
        self.blocks = MIH.make_blocks(LS, B)

    def default(self):
        self.eng.set_mixed(True)
        self.eng.set_screen(1)
        self.eng.set_path(0)

    def plain(self):
        self.eng.set_mixed(False)
        self.eng.set_screen(0)
        self.eng.set_path(1)

    def run(self, blocks, cold):
        if cold:
            self.eng.reset_speculation()
        self.eng.mi_all_pairs(np.ascontiguousarray(blocks, dtype=np.int32), SR_DIST, RETAIN, self.approx)
        return self.eng.links(0), self.eng.links(1), self.eng.block_stats()


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.eng.close()


def same(x, y, what):
    for which in (0, 1):
        for a, b in zip(x[which], y[which]):
            assert np.array_equal(a, b), (what, "sr" if which == 0 else "lr")
    for k in ("n_lr_total", "n_lr_kept", "n_sr", "disc_thresh"):
        assert np.array_equal(x[2][k], y[2][k]), (what, k)


def check(ctx, blocks, what, min_lr=1):
    """plain cold == default cold == default warm == default cold again, row for row"""
    ctx.plain()
    ref = ctx.run(blocks, True)
    assert len(ref[1][2]) >= min_lr, what
    ctx.default()
    c0 = ctx.eng.path_report()
    same(ref, ctx.run(blocks, True), (what, "cold"))
    same(ref, ctx.run(blocks, False), (what, "warm"))
    same(ref, ctx.run(blocks, True), (what, "cold again"))
    c1 = ctx.eng.path_report()
    return ref, {k: c1[k] - c0[k] for k in c1 if isinstance(c1[k], int)}


def is_diag(b):
    return (b[:, 0] == b[:, 2]) & (b[:, 1] == b[:, 3])


def test_whole_list_probes_both_kinds_and_plans_spans_up_front(ctx):
    """The ordinary pass: a diagonal block first (its probe is waited for), the off-diagonal probe collected behind it, spans planned on the
    guess that probe is expected to bring — and they do run as spans in the cold pass."""
    s0 = ctx.eng.span_report()
    _, d = check(ctx, ctx.blocks, "whole list", min_lr=100_000)
    s1 = ctx.eng.span_report()
    assert d["probe_blocks"] >= 4, d            # two cold passes, both kinds sampled in each
    assert s1["spans"] - s0["spans"] >= 3, (s0, s1)


def test_only_diagonal_blocks(ctx):
    check(ctx, ctx.blocks[is_diag(ctx.blocks)], "diagonal blocks only")


def test_only_off_diagonal_blocks(ctx):
    """The first item is off-diagonal: the one probe there is runs on slot 0's buffers and is waited for."""
    check(ctx, ctx.blocks[~is_diag(ctx.blocks)], "off-diagonal blocks only", min_lr=100_000)


def test_one_block_of_each_kind(ctx):
    check(ctx, ctx.blocks[:1], "one diagonal block")
    check(ctx, ctx.blocks[1:2], "one off-diagonal block")


def test_first_off_diagonal_block_too_small_for_a_probe(ctx):
    """No off-diagonal guess will come from a probe (3000 x 3000 = 9 M pairs < 16 M): the plan must not count on one — the span candidates
    behind the small block run block by block on the guess the first finished blocks leave, exactly as before."""
    small = np.array([[1, 3000, 8001, 11000]], dtype=np.int32)
    rest = np.array([b for b in ctx.blocks if not (b[0] == 1 and b[2] == 8001)], dtype=np.int32)   # (the 8000 x 8000 block the small one lies in stays out)
    blocks = np.concatenate([rest[:1], small, rest[1:]])
    assert is_diag(blocks)[0] and not is_diag(blocks)[1]
    check(ctx, blocks, "small first off-diagonal block", min_lr=100_000)


def test_shares_of_a_deal_as_phases_on_one_context(ctx):
    """What a rank of four does: its share of the blocks, call after call on one context (every call starts cold in the job: reset before each)."""
    shares = deal_blocks(ctx.blocks, 4)
    assert sum(len(s) for s in shares) == len(ctx.blocks)
    for rk, idx in enumerate(shares):
        check(ctx, ctx.blocks[idx], ("share", rk))
    # and without a reset between the shares: the guesses of one phase serve the next
    ctx.plain()
    refs = [ctx.run(ctx.blocks[idx], True) for idx in shares]
    ctx.default()
    ctx.eng.reset_speculation()
    for rk, idx in enumerate(shares):
        same(refs[rk], ctx.run(ctx.blocks[idx], False), ("phase after phase", rk))


def test_pass_directly_after_set_weights(ctx):
    """ldw_set_weights forgets the guesses: the next pass starts cold without ldw_reset_speculation, with probes of the new weighting."""
    try:
        ctx.eng.set_weights(ctx.hdw_other)
        ctx.plain()
        ref = ctx.run(ctx.blocks, False)
        ctx.default()
        ctx.eng.set_weights(ctx.hdw_other)
        c0 = ctx.eng.path_report()
        same(ref, ctx.run(ctx.blocks, False), "after set_weights")
        assert ctx.eng.path_report()["probe_blocks"] - c0["probe_blocks"] >= 2
        same(ref, ctx.run(ctx.blocks, False), "after set_weights, warm")
    finally:
        ctx.eng.set_weights(ctx.hdw)
        ctx.default()


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import test_cold_start_order as T
c = T.Ctx()
_, d = T.check(c, c.blocks, "no probes", min_lr=100_000)
assert d["probe_blocks"] == 0, d
c.eng.close()
print("child ok")
"""


def test_without_probes_in_a_child_process():
    """LDW_NO_PROBE=1 (read once per process): no guess before the first block has finished, no spans planned on a cold pass."""
    env = dict(os.environ, LDW_NO_PROBE="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "child ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
