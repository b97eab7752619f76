"""What tests/test_caller_stream_gpu.py runs on every stream: one small job through the whole C ABI surface, the oracle checks of its results, and the
caller's streams themselves.  No test lives here.

``run_job`` returns every result as bytes-comparable numpy arrays under fixed names, so that two runs (one on a caller's stream, one on the library's
own) are compared with ``assert_same``: byte for byte, NaNs included.  The checks against oracle/ldw_oracle.py use the project's existing tolerances:
Hamming weights, shared counts and joint counts bit-exact, dense MI within MI_TIGHT, link tables exact against orc.block_links applied to the device's
own dense MI (the assertions of tests/test_fuzz_oracle.py)."""
import contextlib
import ctypes as C
import hashlib
import math
import os

import numpy as np

import ldw_oracle as orc
from ldweaver_amd import _lib as L
from ldweaver_amd import mi as MIH
from ldweaver_amd import plots as P
from ldweaver_amd import tree as T
from ldweaver_amd.synth import synth_alignment

MI_TIGHT = 1e-10       # tests/test_gpu_parity.py: what the 40-bit fixed-point weights deliver
RETAIN = 0.004         # tests/test_apx_tile_runs_gpu.py: below 0.007 of all links the pass speculates on its thresholds
KINDS = ("current", "not_current", "priority", "blocking")


# ------------------------------------------------------------------------------------------------------------------------------
# the problems
# ------------------------------------------------------------------------------------------------------------------------------
def make_problem(name, Ls, N, blk, sr_dist, seed, oracle_blocks, want_spans, workdir):
    syn = synth_alignment(Ls, N, seed=seed)
    st = np.ascontiguousarray(syn["states"])
    POS, paint, g = syn["POS"], syn["paint"], float(syn["g"])
    uqe, r = orc.uqe_r(st)
    rng = np.random.default_rng(seed + 1)
    blocks = np.ascontiguousarray(MIH.make_blocks(Ls, blk), dtype=np.int32)
    approx = MIH.lr_links_approx(POS, g, sr_dist)
    fi = rng.choice(Ls, size=97, replace=False)           # ragged, unordered index lists
    ti = rng.choice(Ls, size=113, replace=False)
    pa, pb = rng.integers(0, Ls, 6), rng.integers(0, Ls, 6)
    thr = 0.1
    hd = orc.hamming_weights(st, thr)
    # the second alignment of the job (65 sequences: the tree and its bootstrap) and the FASTA file (77 x 1531)
    st65 = np.ascontiguousarray(synth_alignment(400, 65, seed=seed + 2)["states"])
    mult = T.bootstrap_multiplicities(400, 5, seed=seed + 3)
    fa = os.path.join(str(workdir), f"{name}_in.fa")
    chars = rng.choice(list("ACGTN-acgt"), size=(77, 1531), p=[0.22, 0.22, 0.22, 0.22, 0.02, 0.02, 0.02, 0.02, 0.02, 0.02])
    with open(fa, "w") as f:
        for k in range(77):
            f.write(f">seq{k} extra words\n{''.join(chars[k])}\n")
    n = 3000
    plot = (np.floor(rng.random(n) * 50000.0) + 1.0, rng.random(n) ** 3, 3.0 + rng.exponential(2.0, n), (rng.random(n) < 0.6).astype(np.uint8),
            rng.integers(0, 2, n).astype(np.uint8))
    return dict(name=name, L=Ls, N=N, blk=blk, sr_dist=float(sr_dist), states=st, POS=POS, paint=paint, g=g, uqe=uqe, r=r, blocks=blocks, approx=approx,
                retain=RETAIN * approx, fi=fi, ti=ti, pa=pa, pb=pb, thr=thr, st65=st65, mult=mult, fasta=fa, fasta_pos=np.arange(1, 1532, 3, dtype=np.int32),
                plot=plot, oracle_blocks=tuple(oracle_blocks), want_spans=bool(want_spans), want={},
                oracle=dict(hd=hd, shared=orc.shared_counts(st), cnt=np.stack([orc.joint_counts(st, int(a), int(b)) for a, b in zip(pa, pb)]),
                            MI=orc.mi_block_faithful(st, hd, r, uqe, fi, ti),
                            MIi=[(i, j, orc.mi_pair_direct(st, hd, r, uqe, int(fi[i]), int(ti[j]))) for i, j in zip(rng.integers(0, 97, 5), rng.integers(0, 113, 5))]))


def small_problem(workdir):
    """2300 SNPs x 130 sequences in blocks of 1000, sr_dist 3000: 3 block ranges, 6 block pairs — diagonal and off-diagonal pairs, the cold first block,
    speculative later blocks, the GEMM of block b + 1 on the GEMM stream beside the epilogue of block b.  Every block pair is checked against the oracle."""
    return make_problem("small", 2300, 130, 1000, 3000.0, 5, range(6), False, workdir)


def span_problem(workdir):
    """The span shape of tests/test_apx_tile_runs_gpu.py: 10240 SNPs x 300 sequences in five blocks of 2048, whose first block row holds a span of
    long-range-only blocks (planned on the warm pass) on the approximate path.  Every block pair is compared with the own-stream context byte for byte;
    the oracle's selection (0.2 to 0.8 s of numpy per block) is applied to the first block row's diagonal block, a block inside the span and the
    corner block that closes the circle."""
    return make_problem("span", 10240, 300, 2048, 20000.0, 72, (0, 2, 4), True, workdir)


# ------------------------------------------------------------------------------------------------------------------------------
# the job
# ------------------------------------------------------------------------------------------------------------------------------
def _file(path):
    with open(path, "rb") as f:
        return np.frombuffer(f.read(), dtype=np.uint8)


def _digest(a):
    return np.frombuffer(hashlib.sha1(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def load(eng, p, hook=None):
    """Alignment, Hamming weights, weights and SNP meta data: what a pass needs."""
    hook = hook or (lambda stage: None)
    eng.set_engine(L.ENGINE_MFMA)
    eng.set_alignment(p["states"], p["blk"])
    hook("set_alignment")
    hd = eng.hamming_weights(int(p["L"] * p["thr"]))
    hook("hamming_weights")
    eng.set_weights(hd)
    eng.set_snp_meta(p["r"], p["uqe"], p["POS"], p["paint"], p["g"])
    hook("set_snp_meta")


def run_pass(eng, p, cold=True):
    if cold:
        eng.reset_speculation()
    eng.mi_all_pairs(p["blocks"], p["sr_dist"], p["retain"], p["approx"])
    return eng.links(0), eng.links(1)


def check_timing(eng, what):
    """ldw_ctx_last_timing: the stage times come from HIP events recorded on the context's stream."""
    t = eng.last_timing()
    assert all(math.isfinite(v) and v >= 0.0 for v in t.values()) and t["total_ms"] > 0.0, (what, t)


def check_links_against_oracle(eng, p, tables, stats, out, what):
    """tests/test_fuzz_oracle.py's assertions: short-range rows in the reference's order with the dense block's bits, long-range rows equal as a set
    with the same threshold — R/computePairwiseMI.R:306-364 applied to the device's own dense MI of the block."""
    (sa, sb, smi), (la, lb, lmi) = tables
    so = np.concatenate([[0], np.cumsum(stats["n_sr"])])
    lo = np.concatenate([[0], np.cumsum(stats["n_lr_kept"])])
    n_sr = n_lr = 0
    for bi in p["oracle_blocks"]:
        fs, fe, ts, te = p["blocks"][bi].tolist()
        f_idx, t_idx = np.arange(fs - 1, fe), np.arange(ts - 1, te)
        if bi not in p["want"]:
            dense = eng.mi_block(f_idx, t_idx)
            p["want"][bi] = (_digest(dense), orc.block_links(dense, f_idx, t_idx, p["POS"], p["paint"], p["g"], p["sr_dist"], p["retain"], p["approx"]))
        dig, want = p["want"][bi]
        if f"dense{bi}" not in out:
            out[f"dense{bi}"] = _digest(eng.mi_block(f_idx, t_idx))
        assert np.array_equal(out[f"dense{bi}"], dig), (what, bi, "the dense MI of the block differs from the run the oracle's tables were made from")
        s0, s1 = so[bi], so[bi + 1]
        assert np.array_equal(sa[s0:s1], want.sr["a"]) and np.array_equal(sb[s0:s1], want.sr["b"]) and np.array_equal(smi[s0:s1], want.sr["MI"]), (what, bi)
        assert stats["n_lr_total"][bi] == want.n_lr_total, (what, bi)
        l0, l1 = lo[bi], lo[bi + 1]
        got = {(int(x), int(y)): float(m) for x, y, m in zip(la[l0:l1], lb[l0:l1], lmi[l0:l1])}
        ref = {(int(x), int(y)): float(m) for x, y, m in zip(want.lr["a"], want.lr["b"], want.lr["MI"])}
        assert got == ref, (what, bi, len(got), len(ref))
        if want.n_lr_total:
            assert stats["disc_thresh"][bi] == want.disc_thresh, (what, bi)
        n_sr += s1 - s0
        n_lr += l1 - l0
    assert n_sr > 1000 and n_lr > 1000, (what, n_sr, n_lr)


def run_job(eng, p, workdir, tag, hook=None):
    """The whole small job on ``eng``.  ``hook(stage)`` is called between the stages (the stream-switching tests change the stream there)."""
    import torch
    hook = hook or (lambda stage: None)
    o, out = p["oracle"], {}
    path = lambda name: os.path.join(str(workdir), f"{p['name']}_{tag}_{name}")
    eng.set_engine(L.ENGINE_MFMA)
    # the alignment, from a device tensor and from the host
    eng.set_alignment(torch.from_numpy(p["states"]).cuda(), p["blk"])
    out["aln_dev"] = eng.get_alignment()
    eng.set_alignment(p["states"], p["blk"])
    out["aln_host"] = eng.get_alignment()
    assert np.array_equal(out["aln_dev"], p["states"]) and np.array_equal(out["aln_host"], p["states"]), tag
    hook("set_alignment")
    out["state_counts"] = eng.state_counts()
    hd, shared = eng.hamming_weights(int(p["L"] * p["thr"]), want_shared=True)
    out["hd"], out["shared"] = hd, shared
    assert np.array_equal(shared, o["shared"]) and np.array_equal(hd, o["hd"]), tag               # bit-exact
    assert np.array_equal(out["state_counts"], orc.acgtn_table(p["states"])), tag
    hook("hamming_weights")
    eng.set_weights(hd)
    eng.set_snp_meta(p["r"], p["uqe"], p["POS"], p["paint"], p["g"])
    hook("set_snp_meta")
    out["MI"] = eng.mi_block(p["fi"], p["ti"], quirk=L.QUIRK_REFERENCE)
    check_timing(eng, (tag, "mi_block"))
    out["MIi"] = eng.mi_block(p["fi"], p["ti"], quirk=L.QUIRK_INTENDED)
    cnt, fix, fb = eng.joint_tables(p["pa"], p["pb"])
    out["cnt"], out["fix"], out["frac_bits"] = cnt, fix, np.array([fb])
    assert np.abs(out["MI"] - o["MI"]).max() < MI_TIGHT, tag
    for i, j, v in o["MIi"]:
        assert abs(out["MIi"][i, j] - v) < MI_TIGHT, (tag, i, j)
    assert np.array_equal(cnt, o["cnt"]), tag                                                     # bit-exact
    hook("mi_block")
    # the pass: overlap on and off, cold and warm, lr_links.tsv streamed while it runs
    s0, p0 = eng.span_report(), eng.path_report()
    for overlap in (True, False):
        eng.set_overlap(overlap)
        for cold in (True, False):
            k = f"pass_{'overlap' if overlap else 'serial'}_{'cold' if cold else 'warm'}"
            if cold:
                eng.reset_speculation()
            eng.lr_stream_begin(path(k + "_lr_links.tsv"), append=False)
            eng.mi_all_pairs(p["blocks"], p["sr_dist"], p["retain"], p["approx"])
            rows, nbytes, nblk = eng.lr_stream_end()
            check_timing(eng, (tag, k))
            tables, stats = (eng.links(0), eng.links(1)), eng.block_stats()
            assert rows == len(tables[1][2]) > 0 and len(tables[0][2]) > 0 and nblk == len(p["blocks"]), (tag, k, rows, nblk)
            out[k + "_stream"] = _file(path(k + "_lr_links.tsv"))
            assert len(out[k + "_stream"]) == nbytes, (tag, k)
            for which, name in ((0, "sr"), (1, "lr")):
                for col, a in zip("abm", tables[which]):
                    out[f"{k}_{name}_{col}"] = a
            for name, a in stats.items():
                out[f"{k}_{name}"] = a
            check_links_against_oracle(eng, p, tables, stats, out, (tag, k))
            hook(k)
    eng.set_overlap(True)
    s1, p1 = eng.span_report(), eng.path_report()
    if p["want_spans"]:      # conditions of the span shape: without them the case is the small shape again
        assert s1["spans"] - s0["spans"] > 0, (tag, s0, s1)
        assert p1["apx_blocks"] - p0["apx_blocks"] > 0, (tag, p1["apx_gate"])
    # the short-range model and ARACNE on the resident table
    S = int(np.ceil(p["sr_dist"])) - 1
    out["sr_qlo"], out["sr_qhi"], out["sr_qn"] = eng.sr_len_quantiles(3, p["sr_dist"], 0.95)
    md = np.full((3, S), 0.01)
    out["sr_excess"] = eng.sr_excess_stats(md)
    shape = np.array([[0.35, 40.0, math.lgamma(0.35) + math.lgamma(40.0) - math.lgamma(40.35)]] * 3)
    n_red, n_pool, mn = eng.sr_pvalues(md, shape, -1.0)
    assert n_red > 0 and n_pool > 0, (tag, n_red, n_pool)
    out["sr_pvalues"] = np.array([n_red, n_pool, mn])
    # (the kept links and the pool are compacted with atomics: their order is not part of the result.  As tests/test_sr_model_edges.py does, the
    # kept links are put in the reference's order — rows inside one cluster first, then by cluster, then table row — and the pool is sorted.)
    red = eng.sr_reduced()
    order = np.lexsort((red["row"], np.where(red["dup"], red["first_clust"], red["clust_c"]), red["dup"]))
    for name, a in red.items():
        out["sr_red_" + name] = a[order]
    pool = eng.sr_pool()
    po = np.lexsort((pool[2], pool[1], pool[0]))
    for name, a in zip("abm", pool):
        out["sr_pool_" + name] = a[po]
    out["sr_aracne"] = eng.aracne_device()[order]
    hook("sr_model")
    # the consumers of the long-range table
    info = eng.lr_tukey(min_links=500)
    assert info["n_red"] > 0, (tag, info)
    out["tukey"] = np.concatenate([info["q13"], info["thresholds"], [float(info["fallback"]), info["n_red"], info["n_pool"]]])
    for name, a in eng.lr_reduced().items():
        out["lr_red_" + name] = a
    out["lr_aracne"] = eng.aracne_device()
    htm, n_pos, red = eng.ldmap(7)
    out["ldmap"], out["ldmap_info"] = htm, np.array([n_pos, red])
    hook("consumers")
    # the tables as files, and one of them read back into the table it came from
    for which, name in ((0, "sr"), (1, "lr")):
        rows, _ = eng.write_links_tsv(which, path(name + "_links.tsv"), append=False)
        assert rows == eng.links_count(which), (tag, name)
        out[name + "_tsv"] = _file(path(name + "_links.tsv"))
    n_sr = eng.links_count(0)
    rows, slow, _ = eng.tsv_read(path("sr_links.tsv"), "\t", 6)
    assert rows == n_sr, (tag, rows, n_sr)
    out["tsv_cols"] = np.stack([eng.tsv_fetch(k, rows) for k in range(6)])
    assert eng.links_load(0, 0, 1, 5) == n_sr, tag
    for col, a in zip("abm", eng.links(0)):
        out["loaded_sr_" + col] = a
    hook("files")
    # one raster
    rgb, st, _, _ = P.debug_panels(eng, *p["plot"], opts=P.plot_opts(L.PLOT_SR_CLUST, 11, False), n_panels=2, W=211, H=97)
    out["raster"], out["raster_kept"] = rgb, np.array([st["kept"], st["dropped"]])
    # the FASTA feeder
    names, lt, counts = eng.fasta_scan(p["fasta"])
    assert len(names) == 77 and lt == 1531 and names[3] == "seq3", tag
    out["fasta_counts"] = np.ascontiguousarray(counts)
    out["fasta_table"] = eng.fasta_encode(p["fasta_pos"])
    out["fasta_aln"] = eng.get_alignment()
    hook("fasta")
    # the tree of 65 sequences and its bootstrap
    eng.set_alignment(p["st65"], p["blk"])
    out["nj_parent"], out["nj_length"] = eng.nj_tree()
    check_timing(eng, (tag, "nj_tree"))
    for name, a in zip(("parent", "length", "support", "rep_parent", "rep_length"), eng.nj_bootstrap(p["mult"], want_trees=True)):
        out["boot_" + name] = a
    return out


def assert_same(got, ref, what):
    """Byte-identical, name by name."""
    assert sorted(got) == sorted(ref), (what, sorted(set(got) ^ set(ref)))
    for k in ref:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        assert a.tobytes() == b.tobytes(), (what, k, f"{int((a.view(np.uint8) != b.view(np.uint8)).sum()) if a.size else 0} bytes differ")


def tables_of(eng):
    return {f"{name}_{col}": a for which, name in ((0, "sr"), (1, "lr")) for col, a in zip("abm", eng.links(which))}


# ------------------------------------------------------------------------------------------------------------------------------
# resources (ldw_resource_report: device blocks [0], free list [1], pinned blocks [2], events [3], streams the library created [4])
# ------------------------------------------------------------------------------------------------------------------------------
def snapshot():
    out = np.zeros(5, dtype=np.int64)
    L.check(L.lib().ldw_resource_report(L.ptr(out)))
    return out


def baseline():
    n = C.c_int64(0)
    L.check(L.lib().ldw_host_trim(None, C.byref(n)))
    return snapshot()


# ------------------------------------------------------------------------------------------------------------------------------
# the caller's streams
# ------------------------------------------------------------------------------------------------------------------------------
class NoRuntime(Exception):
    pass


def _hip_runtime():
    """The HIP runtime torch has loaded into this process, opened by the name it was mapped under."""
    import torch
    torch.cuda.init()
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    if not paths:
        raise NoRuntime("no libamdhip64 is mapped into this process")
    try:
        rt = C.CDLL(paths[0])
        rt.hipStreamCreate.restype = C.c_int
        rt.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        rt.hipStreamDestroy.restype = C.c_int
        rt.hipStreamDestroy.argtypes = [C.c_void_p]
    except (OSError, AttributeError) as e:
        raise NoRuntime(f"{paths[0]} cannot be opened by name: {e}")
    return rt


class CallerStream:
    """One stream of the caller's: ``handle`` for ldw_ctx_set_stream, ``torch`` to queue torch work on it (``with cs.on():``)."""

    def __init__(self, kind):
        import torch
        self.kind, self._rt, self._cm = kind, None, None
        if kind == "blocking":                       # default flags: it synchronises with the null stream, unlike every stream torch makes
            self._rt = _hip_runtime()
            h = C.c_void_p()
            rc = self._rt.hipStreamCreate(C.byref(h))
            assert rc == 0 and h.value, rc
            self.handle = int(h.value)
            self.torch = torch.cuda.ExternalStream(self.handle, device=0)
        else:
            self.torch = torch.cuda.Stream(device=0, priority=-1) if kind == "priority" else torch.cuda.Stream(device=0)
            self.handle = int(self.torch.cuda_stream)
        if kind == "current":                        # the benchmark's set-up: torch's own work runs on it too
            self._cm = torch.cuda.stream(self.torch)
            self._cm.__enter__()

    def on(self):
        import torch
        return torch.cuda.stream(self.torch)

    def works(self):
        """A torch computation queued on the stream gives the right result."""
        import torch
        with self.on():
            t = torch.arange(1000, device="cuda:0", dtype=torch.float64) * 2.0
            s = t.sum()
        self.torch.synchronize()
        return float(s) == 999_000.0

    def close(self):
        """After every context that adopted it is gone."""
        self.torch.synchronize()
        if self._cm is not None:
            self._cm.__exit__(None, None, None)
            self._cm = None
        if self._rt is not None:
            assert self._rt.hipStreamDestroy(C.c_void_p(self.handle)) == 0
            self._rt = None


@contextlib.contextmanager
def caller_stream(kind):
    cs = CallerStream(kind)
    try:
        yield cs
    finally:
        cs.close()


# ------------------------------------------------------------------------------------------------------------------------------
# a producer that is still running when the library is called
# ------------------------------------------------------------------------------------------------------------------------------
class Producer:
    """Plain torch work on the caller's stream — a chain of matmuls — followed by the kernel that writes the input, with nothing between it and the
    library call but the check that it has not finished.  The chain starts at about 20 ms (measured here with torch events, never assumed) and is
    doubled, four times at the most, whenever it was over before the call could be issued."""

    def __init__(self, cs):
        import torch
        self.cs, self.log = cs, []
        with cs.on():
            self.a = torch.randn((2048, 2048), device="cuda:0", dtype=torch.float32) / 64.0
            self.b = self.a.clone()
            self._chain(8)                              # (library handles and work-spaces of the first matmul)
            cs.torch.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(cs.torch)
            self._chain(32)
            e1.record(cs.torch)
            cs.torch.synchronize()
        self.unit_ms = e0.elapsed_time(e1) / 32.0
        self.reps = max(8, int(math.ceil(20.0 / max(self.unit_ms, 1e-4))))

    def _chain(self, n):
        import torch
        for _ in range(n):
            torch.mm(self.a, self.b, out=self.b)
            self.b.clamp_(-1.0, 1.0)

    def run(self, what, write, call):
        """Queue the chain and ``write()`` on the stream, then ``call()`` (the library) while they still run.  Returns what ``call`` returned."""
        import torch
        for attempt in range(5):
            with self.cs.on():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(self.cs.torch)
                self._chain(self.reps)
                write()
                e1.record(self.cs.torch)
            running = not e1.query()
            if running:
                res = call()
            self.cs.torch.synchronize()
            ms = e0.elapsed_time(e1)
            self.log.append((what, self.reps, ms, running))
            print(f"[producer] {self.cs.kind} {what}: {self.reps} matmuls, {ms:.1f} ms on the stream, still running at the call: {running}")
            if running:
                return res
            self.reps *= 2
        raise AssertionError(f"{what}: the producer had always finished before the library call could be issued (last: {self.reps // 2} matmuls): the case is vacuous")
