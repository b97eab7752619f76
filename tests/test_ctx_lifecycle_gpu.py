"""GPU: what a context makes goes with it (pytest -m gpu).  ldw_resource_report counts, process-wide, the device blocks held by live buffers [0], the
released blocks on the free list [1], the pinned host blocks [2], the events [3] and the streams the library created [4].  Other tests of the process
may hold engines (the session's ``engine`` fixture), so every test takes a baseline after ldw_host_trim(NULL) and compares differences.

The job of these tests: 600 SNPs x 130 sequences (Npad = 256, N no multiple of 128) of the synthetic recipe, 50 bp apart, in blocks of 150 — 4 block
ranges, 10 block pairs, more than the 3 pipeline slots: every per-slot buffer, the event pool and the growth of the pinned staging are used."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from ldweaver_amd import _lib as L
from ldweaver_amd import mi as MIH
from ldweaver_amd.engine import Engine
from ldweaver_amd.synth import synth_alignment

pytestmark = pytest.mark.gpu

LS, N, BLK, SR_DIST = 600, 130, 150, 2000.0
OWNED = (0, 2, 3, 4)          # the slots a context's share of which is gone after ldw_ctx_destroy
GREP_NAMES = ("pos1", "pos2", "len", "ARACNE", "MI", "pos1_ann", "pos2_ann", "links")


def snapshot():
    out = np.zeros(5, dtype=np.int64)
    L.check(L.lib().ldw_resource_report(L.ptr(out)))
    return out


def baseline():
    n = C.c_int64(0)
    L.check(L.lib().ldw_host_trim(None, C.byref(n)))
    return snapshot()


def owned(s):
    return [int(s[k]) for k in OWNED]


@pytest.fixture(scope="module")
def job():
    syn = synth_alignment(LS, N, seed=47)
    POS = (1 + 50 * np.arange(LS)).astype(np.int32)
    g = float(50 * LS + 10_000)
    blocks = MIH.make_blocks(LS, BLK)
    assert len(blocks) == 10 and syn["states"].shape == (LS, N)
    return dict(states=syn["states"], POS=POS, paint=syn["paint"], g=g, blocks=blocks, retain=0.02 * LS * LS / 2,
                approx=MIH.lr_links_approx(POS, g, SR_DIST))


def load(eng, d):
    eng.set_alignment(d["states"], BLK)
    uqe = (eng.state_counts() > 0).T.astype(np.float64)
    eng.set_weights(eng.hamming_weights(int(LS * 0.1)))
    eng.set_snp_meta(uqe.sum(axis=1), uqe, d["POS"], d["paint"], d["g"])


def run_pass(eng, d):
    eng.mi_all_pairs(d["blocks"], SR_DIST, d["retain"], d["approx"])
    return eng.links(0), eng.links(1)


def whole_job(eng, d, tmp):
    """The pass and every consumer that keeps state in the context: the short-range model, the link-table writer and reader, the search of an annotated
    file, the alignment writer, the FASTA scan, a timed plot."""
    load(eng, d)
    sr, lr = run_pass(eng, d)
    assert len(sr[2]) > 0 and len(lr[2]) > 0
    eng.sr_len_quantiles(3, SR_DIST, 0.95)
    md = np.full((3, int(SR_DIST) - 1), 0.01)
    eng.sr_excess_stats(md)
    shape = np.array([[0.35, 40.0, math.lgamma(0.35) + math.lgamma(40.0) - math.lgamma(40.35)]] * 3)
    eng.sr_pvalues(md, shape, -1.0)
    rows, _ = eng.write_links_tsv(0, str(tmp / "sr.tsv"), append=False)
    assert rows == len(sr[2]) and eng.tsv_read(tmp / "sr.tsv", "\t", 6)[0] == rows
    np.testing.assert_allclose(eng.tsv_fetch(5, rows), sr[2], rtol=1e-12)          # (the writer prints 15 significant digits)
    ann = tmp / "ann.tsv"
    ann.write_text("\t".join(GREP_NAMES) + "\n" + "8\t9\t1\t1\t0.25\tabc:1\tdnaA:3\tnsXns\n" + "9\t9\t1\t0\t0.125\tfolA:1\tgyrB:3\tsyXsy\n")
    assert eng.links_grep(str(ann), ["abc"])["row"].tolist() == [0]
    assert eng.write_alignment(tmp / "out.fa", np.arange(0, LS, 7), [f"s{k}" for k in range(N)]) > 0
    rng = np.random.default_rng(5)
    fa = tmp / "in.fa"
    fa.write_text("".join(f">r{k}\n{''.join(rng.choice(list('ACGT'), 200))}\n" for k in range(20)))
    names, lt, _ = eng.fasta_scan(fa)
    assert len(names) == 20 and lt == 200
    caps = np.array([(2, 2, 50, 40, 3, 0x3366CC, 255)], dtype=Engine.CAPSULE)
    assert eng.plot_capsules(caps, 64, 48, timings=True)[0].shape == (48, 64, 3)
    return sr, lr


def test_everything_a_context_makes_goes_with_it(job, tmp_path):
    base = baseline()
    for cycle in (0, 1):          # (the second cycle: nothing is left in process-wide statics)
        eng = Engine(0)
        whole_job(eng, job, tmp_path)
        held = snapshot()
        assert all(h > b for h, b in zip(owned(held), owned(base))), (cycle, base, held)
        eng.close()
        after = snapshot()
        print(f"cycle {cycle}: baseline {base.tolist()} in use {held.tolist()} after close {after.tolist()}")
        assert owned(after) == owned(base), (cycle, base, held, after)


def test_create_refuses_a_device_out_of_range_and_leaves_nothing():
    base = baseline()
    ctx = C.c_void_p()
    assert L.lib().ldw_ctx_create(1 << 20, C.byref(ctx)) == L.LDW_ERR_ARG and not ctx.value
    assert snapshot().tolist() == base.tolist()


def test_the_free_list_is_accounted_for():
    """states [70 000][1024] is 68 MiB: a block that goes to the free list when the context goes (unless LDW_DEVPOOL_GB = 0 switches the list off)."""
    base = baseline()
    assert base[1] == 0
    states = np.random.default_rng(3).integers(0, 5, size=(70_000, 1_000), dtype=np.uint8)
    eng = Engine(0)
    eng.set_alignment(states, BLK)
    assert snapshot()[0] > base[0]
    eng.close()
    after = snapshot()
    pool_off = float(os.environ.get("LDW_DEVPOOL_GB", "48")) <= 0
    print(f"baseline {base.tolist()} after close {after.tolist()} (free list {'off' if pool_off else 'on'})")
    assert after[0] == base[0] and (after[1] == 0 if pool_off else after[1] >= 1), (base, after)
    n = C.c_int64(0)
    L.check(L.lib().ldw_host_trim(None, C.byref(n)))
    assert snapshot()[1] == 0 and (pool_off or n.value >= 70_000 * 1024)


def test_an_adopted_stream_survives(job):
    import torch
    base = baseline()
    s = torch.cuda.Stream(device=0)
    eng = Engine(0, stream=s.cuda_stream)
    if os.environ.get("LDW_NO_PREPARE") is None:
        assert snapshot()[4] == base[4] + 3      # (its own main stream went when the caller's came: copy, GEMM and writer streams are left)
    load(eng, job)
    sr, lr = run_pass(eng, job)
    assert len(sr[2]) > 0 and len(lr[2]) > 0
    eng.close()
    with torch.cuda.stream(s):
        t = torch.arange(1000, device="cuda:0", dtype=torch.float64) * 2.0
    s.synchronize()
    assert float(t.sum()) == 999_000.0
    assert owned(snapshot()) == owned(base)


def test_reserve_without_a_pass():
    """Both side threads are joined and the pinned staging of ldw_ctx_reserve is freed by a destroy that follows at once."""
    base = baseline()
    eng = Engine(0)
    eng.reserve(LS, N, BLK)
    eng.reserve(LS, N, BLK)
    eng.close()
    assert owned(snapshot()) == owned(base)


def test_two_contexts_one_destroyed(job):
    base = baseline()
    a, b = Engine(0), Engine(0)
    load(a, job)
    load(b, job)
    ra, rb = run_pass(a, job), run_pass(b, job)
    for which in (0, 1):
        assert all(np.array_equal(x, y) for x, y in zip(ra[which], rb[which]))
    a.close()
    again = run_pass(b, job)
    for which in (0, 1):
        assert len(rb[which][2]) > 0 and all(np.array_equal(x, y) for x, y in zip(rb[which], again[which])), which
    b.close()
    assert owned(snapshot()) == owned(base)


def test_trim_then_read_again(tmp_path):
    """host_trim gives the reader's pinned pair back (at least the reported pinned_bytes); the next read of the same file makes it anew."""
    rng = np.random.default_rng(9)
    tab = rng.integers(1, 10**6, size=(500, 3))
    p = tmp_path / "t.tsv"
    p.write_text("".join(f"{a}\t{b}\t{c / 1024}\n" for a, b, c in tab))
    base = baseline()
    with Engine(0) as eng:
        assert eng.tsv_read(p, "\t", 3)[0] == 500
        first = [eng.tsv_fetch(k, 500) for k in range(3)]
        pinned = eng.tsv_stats()["pinned_bytes"]
        assert pinned > 0 and eng.host_trim() >= pinned and eng.tsv_stats()["pinned_bytes"] == 0
        assert eng.tsv_read(p, "\t", 3)[0] == 500
        assert all(np.array_equal(x, eng.tsv_fetch(k, 500)) for k, x in enumerate(first))
        assert np.array_equal(first[0], tab[:, 0].astype(np.float64)) and np.array_equal(first[2], tab[:, 2] / 1024)
    assert owned(snapshot()) == owned(base)
