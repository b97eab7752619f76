"""GPU: the engine on a stream the caller owns, the way bench.py runs it (pytest -m gpu).

Every other test of the suite uses ``Engine(0)``: the library's own hipStreamNonBlocking stream.  The benchmark hands the library a torch stream that
is torch's current one.  Here the contract of include/ldweaver_amd.h ("Streams and synchronisation", "Device memory handed out", ldw_ctx_set_stream)
is run on four kinds of caller stream (caller_stream_job.KINDS): a torch stream that is current, one that is not, one of high priority, and a
blocking stream made with hipStreamCreate on the runtime torch has loaded.

  A  a whole small job (caller_stream_job.run_job: every stage from set_alignment to the bootstrap tree) equals the oracle where the project has
     one, at its existing tolerances, and equals the same job on an own-stream context byte for byte; on two shapes.
  B  the ordering contract against work the caller has queued in front of a call and never waited for: a producer that is provably still running
     when the library is called (caller_stream_job.Producer).
  C  ldw_ctx_set_stream between jobs, between the stages of a job, inside an open link pass and while a tsv writer is open; what it does to the
     library's resource counts; two contexts on two caller streams and on one.

No tolerance is new.  No case may skip but the blocking stream, when the HIP runtime cannot be opened by name."""
import contextlib
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import caller_stream_job as J
import ldw_oracle as orc
from ldweaver_amd import _lib as L
from ldweaver_amd.engine import Engine

pytestmark = pytest.mark.gpu

OWNED = (0, 2, 3, 4)          # the slots of ldw_resource_report a context's share of which is gone after ldw_ctx_destroy


@contextlib.contextmanager
def stream_of(kind):
    try:
        cs = J.CallerStream(kind)
    except J.NoRuntime as e:
        assert kind == "blocking"
        pytest.skip(f"a blocking stream needs hipStreamCreate of the runtime torch loaded: {e}")
    try:
        yield cs
    finally:
        cs.close()


class _Refs:
    """Per shape: the problem and the job's results on an own-stream context, made once (with every oracle check) and never changed."""

    def __init__(self, work):
        self.work, self.made = work, {}

    def get(self, shape):
        if shape not in self.made:
            p = (J.small_problem if shape == "small" else J.span_problem)(self.work)
            with Engine(0) as eng:
                ref = J.run_job(eng, p, self.work, "own")
            self.made[shape] = (p, ref)
        return self.made[shape]


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("caller_stream")


@pytest.fixture(scope="module")
def refs(work):
    return _Refs(work)


def owned(s):
    return [int(s[k]) for k in OWNED]


# ------------------------------------------------------------------------------------------------------------------------------
# A: a whole job on a caller's stream
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["small", "span"])
@pytest.mark.parametrize("kind", J.KINDS)
def test_a_whole_job_on_a_caller_stream_equals_the_oracle_and_the_own_stream_context(refs, work, kind, shape):
    p, ref = refs.get(shape)
    with stream_of(kind) as cs:
        with Engine(0, stream=cs.handle) as eng:
            got = J.run_job(eng, p, work, kind)
        assert cs.works()                                 # an adopted stream is never destroyed
    J.assert_same(got, ref, (kind, shape))


# ------------------------------------------------------------------------------------------------------------------------------
# B: the ordering contract against work the caller has queued
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=J.KINDS)
def bctx(request, refs, work):
    """A context on a caller's stream that holds a finished pass, the geometry of the short-range model and a table read from a file."""
    import torch
    p, _ = refs.get("small")
    with stream_of(request.param) as cs:
        eng = Engine(0, stream=cs.handle)
        J.load(eng, p)
        J.run_pass(eng, p)
        eng.sr_len_quantiles(3, p["sr_dist"], 0.95)
        path = str(work / f"b_{request.param}_sr.tsv")
        rows, _ = eng.write_links_tsv(0, path, append=False)
        assert eng.tsv_read(path, "\t", 6)[0] == rows > 0
        torch.cuda.synchronize()
        yield SimpleNamespace(cs=cs, eng=eng, p=p, prod=J.Producer(cs), kind=request.param, rows=rows)
        eng.close()


def on_the_null_stream(*tensors):
    """Copies of device tensors made by torch's null stream and brought to the host by it: no stream of the test or the library is waited for."""
    import torch
    with torch.cuda.stream(torch.cuda.default_stream(0)):
        return [t.clone().cpu().numpy() for t in tensors]


def test_b_device_alignment_filled_by_a_producer_still_running(bctx):
    """ldw_set_alignment(on_device = 1) through the C ABI (Engine.set_alignment waits for the whole device first and would hide the case): the
    tensor is filled on the caller's stream behind the matmul chain; the library's read is ordered behind it by the stream alone."""
    import torch
    p, cs = bctx.p, bctx.cs
    src = torch.from_numpy(p["states"]).cuda()
    with cs.on():
        t = torch.full(p["states"].shape, 7, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    with Engine(0, stream=cs.handle) as eng:
        bctx.prod.run("ldw_set_alignment(on_device)", lambda: t.copy_(src),
                      lambda: L.check(L.lib().ldw_set_alignment(eng._ctx, L.ptr(t), p["L"], p["N"], 1)))
        eng.L, eng.N = p["L"], p["N"]
        assert np.array_equal(eng.get_alignment(), p["states"])
        assert np.array_equal(eng.hamming_weights(int(p["L"] * p["thr"])), p["oracle"]["hd"])


def test_b_queue_only_twins_between_a_producer_and_a_consumer(bctx, kat):
    """ldw_fast_hadamard(on_device = 1) and ldw_acgtn2num_dev only queue their kernel: input written on the stream in front of them, a torch
    reduction and a copy queued behind them, no ldw_ctx_sync anywhere.  Against src/computeMI.cpp:19 and the ACGTN2num rule as the oracle
    states them, at the tolerance of test_elementwise_twins (the device log() may differ from libm in the last ulp; the mask is exact)."""
    import torch
    cs, ctx = bctx.cs, bctx.eng._ctx
    flat = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1, order="F"))
    ops_h = [kat[f"op_{k}"] for k in ("den", "uq", "pxy", "pxpy", "RXY", "pXrX", "pYrY")]
    ops_d = [torch.from_numpy(flat(a)).cuda() for a in ops_h]
    mi0_d = torch.from_numpy(flat(kat["MI0"])).cuda()
    mi_d = torch.full_like(mi0_d, float("nan"))
    torch.cuda.synchronize()

    def hadamard():
        L.check(L.lib().ldw_fast_hadamard(ctx, L.ptr(mi_d), *[L.ptr(o) for o in ops_d], mi_d.numel(), 1))
        with cs.on():
            return mi_d.sum(), mi_d.clone()

    s, c = bctx.prod.run("ldw_fast_hadamard(on_device)", lambda: mi_d.copy_(mi0_d), hadamard)
    want = kat["MI0"].copy()
    orc.fast_hadamard(want, *ops_h)
    np.testing.assert_allclose(c.cpu().numpy().reshape(want.shape, order="F"), want, rtol=1e-15, atol=1e-15)
    assert float(s) == float(c.sum())
    # ACGTN2num: nv is 5 x L column-major, ref the first character of every string ("" is NUL: the column stays)
    ref = b"".join(str(x)[:1].encode("latin1") or b"\0" for x in kat["ref_chars"])
    n = len(ref)
    ref_d = torch.from_numpy(np.frombuffer(ref, dtype=np.uint8).copy()).cuda()
    ones = torch.ones(5 * n, dtype=torch.float64, device="cuda:0")
    nv_d = torch.full_like(ones, float("nan"))
    torch.cuda.synchronize()

    def acgtn():
        L.check(L.lib().ldw_acgtn2num_dev(ctx, L.ptr(nv_d), L.ptr(ref_d), n))
        with cs.on():
            return nv_d.sum(), nv_d.clone()

    s, c = bctx.prod.run("ldw_acgtn2num_dev", lambda: nv_d.copy_(ones), acgtn)
    want = np.ones((5, n), order="F")
    orc.acgtn2num(want, list(kat["ref_chars"]))
    assert np.array_equal(c.cpu().numpy(), want.reshape(-1, order="F")) and np.array_equal(want, kat["nv"])
    assert float(s) == float(want.sum())


def test_b_synchronising_calls_are_complete_when_they_return(bctx):
    """Calls that write caller device memory synchronise before they return: the result is read by torch's null stream at once, with no wait of
    the test's, and equals the host route's.  In front of every call the stream holds the running producer, which ends by overwriting the
    output: a call that returned early would leave its NaNs (or nothing) there."""
    import torch
    eng, p, cs, prod = bctx.eng, bctx.p, bctx.cs, bctx.prod
    lib, ctx = L.lib(), eng._ctx
    dev = torch.device("cuda", 0)
    junk = lambda *ts: (lambda: [t.fill_(float("nan")) if t.is_floating_point() else t.fill_(-1) for t in ts])
    # mi_block(out = device tensor)
    want = eng.mi_block(p["fi"], p["ti"])
    out = torch.zeros(want.size, dtype=torch.float64, device=dev)
    got, = prod.run("ldw_mi_block(on_device)", junk(out), lambda: on_the_null_stream(eng.mi_block(p["fi"], p["ti"], out=out)))
    assert np.array_equal(got.reshape(want.shape, order="F"), want)
    # links(which, device_tensors = True) and links_view
    for which in (0, 1):
        host = eng.links(which)
        scratch = torch.zeros(1 << 20, dtype=torch.float64, device=dev)
        got = prod.run(f"ldw_links_fetch({which}, on_device)", junk(scratch), lambda: on_the_null_stream(*eng.links(which, device_tensors=True)))
        assert all(np.array_equal(x, y) for x, y in zip(got, host)) and len(host[2]) > 0
        got = prod.run(f"ldw_links_device_ptrs({which})", junk(scratch), lambda: on_the_null_stream(*eng.links_view(which)))
        assert all(np.array_equal(x, y) for x, y in zip(got, host))
    # sr_tail_extract(on_device = 1), through the C ABI (Engine.sr_tail_extract waits for the whole device between its two calls)
    S = int(np.ceil(p["sr_dist"])) - 1
    lower = np.zeros((3, S))
    cnt_h, mi_h = eng.sr_tail_extract(lower)
    assert len(mi_h) > 0
    mi_d = torch.zeros(len(mi_h), dtype=torch.float64, device=dev)
    cnt = np.zeros((S, 3), dtype=np.int64)
    n = C.c_int64(0)

    def tail():
        L.check(lib.ldw_sr_tail_extract(ctx, 3, S, L.ptr(lower), L.ptr(cnt), L.ptr(mi_d), len(mi_h), 1, C.byref(n)))
        return on_the_null_stream(mi_d)

    got, = prod.run("ldw_sr_tail_extract(on_device)", junk(mi_d), tail)
    # (the values come grouped by (len, cluster); inside a group they are placed with an atomic cursor: sorted there before they are compared)
    gid = np.repeat(np.arange(cnt_h.size), cnt_h.ravel())
    in_groups = lambda v: v[np.lexsort((v, gid))]
    assert n.value == len(mi_h) and np.array_equal(cnt, cnt_h) and np.array_equal(in_groups(got), in_groups(mi_h))    # tsv_fetch(on_device = 1)
    col_h = eng.tsv_fetch(5, bctx.rows)
    col_d = torch.zeros(bctx.rows, dtype=torch.float64, device=dev)

    def fetch():
        L.check(lib.ldw_tsv_fetch(ctx, 5, L.ptr(col_d), bctx.rows, 1))
        return on_the_null_stream(col_d)

    got, = prod.run("ldw_tsv_fetch(on_device)", junk(col_d), fetch)
    assert np.array_equal(got, col_h)


def test_b_import_of_tables_produced_behind_a_running_producer(bctx):
    """ldw_links_import(on_device = 1) through the C ABI (Engine.links_import waits for the whole device first): the three columns are written on
    the caller's stream behind the matmul chain."""
    import torch
    eng, cs = bctx.eng, bctx.cs
    want = eng.links(1)
    n = len(want[2])
    src = [torch.from_numpy(np.ascontiguousarray(x[::-1])).cuda() for x in want]          # (another table than the resident one: reversed)
    with cs.on():
        dst = [torch.zeros_like(x) for x in src]
    torch.cuda.synchronize()
    try:
        bctx.prod.run("ldw_links_import(on_device)", lambda: [d.copy_(s) for d, s in zip(dst, src)],
                      lambda: L.check(L.lib().ldw_links_import(eng._ctx, 1, L.ptr(dst[0]), L.ptr(dst[1]), L.ptr(dst[2]), n, 1)))
        got = eng.links(1)
        assert n > 0 and all(np.array_equal(x, y[::-1]) for x, y in zip(got, want))
    finally:
        eng.links_import(1, *want)


# ------------------------------------------------------------------------------------------------------------------------------
# C: switching and ownership
# ------------------------------------------------------------------------------------------------------------------------------
def test_c_one_context_through_three_streams(refs, work):
    """set_stream(S1), the job, set_stream(S2), the job, set_stream(None), the job: each equals the own-stream context's.  Adopting a stream takes
    the library's stream count down by one (its own main stream goes), going from one caller's stream to another leaves it, set_stream(None) makes
    a main stream again; no event is made or lost by a switch; after close() the context's share of the counts is gone, and both caller streams
    still work."""
    p, ref = refs.get("small")
    base = J.baseline()
    with stream_of("not_current") as s1, stream_of("priority") as s2:
        eng = Engine(0)

        def switch(to, d_streams):
            before = J.snapshot()
            eng.set_stream(to)
            after = J.snapshot()
            assert after[4] - before[4] == d_streams and after[3] == before[3], (before, after)

        switch(s1.handle, -1)
        got1 = J.run_job(eng, p, work, "c_s1")
        switch(s2.handle, 0)
        got2 = J.run_job(eng, p, work, "c_s2")
        switch(None, +1)
        got3 = J.run_job(eng, p, work, "c_own")
        eng.close()
        after = J.snapshot()
        assert owned(after) == owned(base), (base, after)
        assert s1.works() and s2.works()
    for tag, got in (("S1", got1), ("S2", got2), ("own again", got3)):
        J.assert_same(got, ref, tag)


def test_c_switching_between_the_stages_of_one_job(refs, work):
    """The stream changes right after ldw_ctx_create (what Engine(.., stream = ..) does: the side thread that loads the kernels may still run; it
    touches no stream of the context), after hamming_weights, after set_snp_meta and in front of the consumers."""
    p, ref = refs.get("small")
    with stream_of("not_current") as s1, stream_of("priority") as s2:
        eng = Engine(0)
        eng.set_stream(s1.handle)
        to = {"hamming_weights": s2.handle, "set_snp_meta": None, "sr_model": s1.handle}
        got = J.run_job(eng, p, work, "c_stages", hook=lambda stage: eng.set_stream(to[stage]) if stage in to else None)
        eng.close()
        assert s1.works() and s2.works()
    J.assert_same(got, ref, "switched between the stages")


def test_c_switching_inside_an_open_pass_and_an_open_writer(refs, work):
    """ldw_ctx_set_stream drains the old main stream and the context's helper streams, so it is safe between any two calls: between
    ldw_links_begin and ldw_links_end the tables are those of the same block-wise pass without a switch; around a pass whose lr_links.tsv is
    being streamed, and between ldw_write_links_tsv_begin and _end, the files are the own-stream context's."""
    p, ref = refs.get("small")
    with stream_of("not_current") as s1, stream_of("priority") as s2, Engine(0) as eng:
        J.load(eng, p)

        def blockwise(switch_at):
            eng.reset_speculation()
            eng.links_begin(len(p["blocks"]))
            for bi, (fs, fe, ts, te) in enumerate(p["blocks"].tolist()):
                if bi in switch_at:
                    eng.set_stream(switch_at[bi])
                eng.mi_block_links(np.arange(fs - 1, fe), np.arange(ts - 1, te), p["sr_dist"], p["retain"], p["approx"])
            eng.links_end()
            return dict(J.tables_of(eng), **eng.block_stats())

        plain = blockwise({})
        assert len(plain["sr_m"]) > 0 and len(plain["lr_m"]) > 0
        J.assert_same(blockwise({1: s1.handle, 3: s2.handle, 5: None}), plain, "switched between the blocks of an open pass")
        # the streaming writer: opened on one stream, the pass on a second, closed on a third
        f1 = str(work / "c_open_lr_links.tsv")
        eng.reset_speculation()
        eng.lr_stream_begin(f1, append=False)
        eng.set_stream(s1.handle)
        eng.mi_all_pairs(p["blocks"], p["sr_dist"], p["retain"], p["approx"])
        eng.set_stream(s2.handle)
        rows, _, nblk = eng.lr_stream_end()
        assert rows == eng.links_count(1) and nblk == len(p["blocks"])
        assert J._file(f1).tobytes() == ref["pass_overlap_cold_stream"].tobytes()
        for k, a in J.tables_of(eng).items():
            assert a.tobytes() == ref["pass_overlap_cold_" + k].tobytes(), k
        # the asynchronous writer holds a host copy of the table
        f2 = str(work / "c_open_lr.tsv")
        eng.write_links_tsv_begin(1, f2, append=False)
        eng.set_stream(None)
        assert eng.write_links_tsv_end()[0] == rows
        assert J._file(f2).tobytes() == ref["lr_tsv"].tobytes()
        assert s1.works() and s2.works()


def test_c_two_contexts_on_two_caller_streams_and_on_one(refs):
    """ldw_mi_all_pairs_multi with two contexts, each on a caller's stream of its own, assembles the tables of one own-stream context.  Two
    contexts may also adopt the SAME caller's stream: their work is then serialised on it, in the order of the calls, and the results do not
    change — used one after the other and together in one multi pass."""
    p, ref = refs.get("small")
    want = {k: ref["pass_overlap_cold_" + k] for k in ("sr_a", "sr_b", "sr_m", "lr_a", "lr_b", "lr_m")}
    kw = dict(sr_dist=p["sr_dist"], lr_retain_links=p["retain"], lr_links_approx=p["approx"])
    with stream_of("not_current") as s1, stream_of("priority") as s2:
        a, b = Engine(0, stream=s1.handle), Engine(0, stream=s2.handle)
        try:
            J.load(a, p)
            J.load(b, p)
            for tag in ("two streams", "one stream"):
                for e in (a, b):
                    e.reset_speculation()
                info = Engine.mi_all_pairs_multi([a, b], p["blocks"], **kw)
                assert sorted(set(info["owner"].tolist())) == [0, 1], (tag, info["owner"])
                J.assert_same(J.tables_of(a), want, ("multi", tag))
                for e in (b, a):      # (alternating on the shared stream)
                    J.run_pass(e, p)
                    J.assert_same(J.tables_of(e), want, ("one after the other", tag))
                b.set_stream(s1.handle)
        finally:
            a.close()
            b.close()
        assert s1.works() and s2.works()
